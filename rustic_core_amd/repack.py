"""Repack and copy on the device: kept blobs of old packs in HBM opened,
decoded, compressed at the destination's level, sealed with the destination's
key and written into new packs (read.read_blobs, compress.process_blobs and
rcdc_pack_build_raw_multi / rcdc_copy_ranges / rcdc_sha256_chunks in
include/rcdc.h).

Reference: ``BlobCopier`` (crates/core/src/blob/packer.rs:908-1054) over
``CopyPackBlobs`` (:880-906) -- what ``prune``'s repack
(commands/prune.rs:1320-1323, :1384-1430) and ``copy``
(commands/copy.rs:91-173) move blobs with; ``--repack-uncompressed`` of a
version-1 repository is the same path.  ``plan_copy`` / ``plan_repack`` are
the host half (sorting, dedup of used ids, read coalescing); ``BlobCopier``
is the executor: per group of ranges one read_blobs call, one process_blobs
call and the packer (``Packer`` :259-289, ``RawPacker::add_raw`` /
``should_save`` :479-493, :659-671).  No CPU fallback.
"""
from __future__ import annotations

import copy as _copy
from dataclasses import dataclass
from typing import Callable, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .errors import ErrorKind, RusticError
from .index import IndexBlob, IndexPack, rustic_time
from .pack import (PACK_BLOB, PackSizer, build_packs_multi, copy_ranges, group_blobs_open,
                   index_entries, make_blobs, pack_layout, random_nonces)
from .restore import BlobLocation, can_coalesce, data_length


class CopyPackBlobs(NamedTuple):
    """packer.rs:880-906 with its BlobLocations (blob.rs:155-159) flattened:
    one read of ``length`` bytes at ``offset`` of pack ``pack_id`` and the
    blobs it holds, ``blobs``: [(BlobLocation, blob id)]."""
    pack_id: bytes
    offset: int
    length: int
    blobs: list

    @classmethod
    def from_index_entry(cls, pack_id: bytes, index_blob) -> "CopyPackBlobs":
        """CopyPackBlobs::from_index_entry (packer.rs:887-892)."""
        bl = BlobLocation(int(index_blob.offset), int(index_blob.length),
                          int(index_blob.uncompressed_length or 0))
        return cls(bytes(pack_id), bl.offset, bl.length, [(bl, bytes(index_blob.id))])

    def coalesce(self, other: "CopyPackBlobs") -> Optional["CopyPackBlobs"]:
        """CopyPackBlobs::coalesce (packer.rs:896-905): the merged read, or
        None -- the same pack, and restore.can_coalesce's rule."""
        if (self.pack_id == other.pack_id
                and can_coalesce(self.offset, self.length, other.offset, other.length)):
            return CopyPackBlobs(self.pack_id, self.offset,
                                 other.offset + other.length - self.offset,
                                 self.blobs + other.blobs)
        return None


def _coalesced(items: Iterable[CopyPackBlobs]) -> List[CopyPackBlobs]:
    out: List[CopyPackBlobs] = []
    for cur in items:
        merged = out[-1].coalesce(cur) if out else None
        if merged is not None:
            out[-1] = merged
        else:
            out.append(cur)
    return out


def _blob_order(b):
    """IndexBlob's order (indexfile.rs: by BlobLocation, offset first)."""
    return (int(b.offset), int(b.length), int(b.uncompressed_length or 0), int(b.type),
            bytes(b.id))


def plan_copy(entries: Iterable[Tuple[bytes, IndexBlob]]) -> List[CopyPackBlobs]:
    """copy_blobs' plan (copy.rs:150-159): ``entries`` -- (pack id, IndexBlob)
    per blob to copy -- sorted by pack id, then offset (length, uncompressed
    length and id break ties, which the reference's unstable sort leaves
    open), neighbours coalesced."""
    es = sorted(((bytes(p), b) for p, b in entries), key=lambda e: (e[0],) + _blob_order(e[1]))
    return _coalesced(CopyPackBlobs.from_index_entry(p, b) for p, b in es)


def plan_repack(index_pack, used_ids: set) -> List[CopyPackBlobs]:
    """One pack of prune's repack (prune.rs:1320-1323, :1408-1417): the
    blobs of ``index_pack`` whose id is in ``used_ids``, each id taken out of
    the set as it is kept (a blob that two packs hold is saved once, by the
    pack that comes first), sorted in IndexBlob order and coalesced."""
    kept = []
    for b in index_pack.blobs:
        if bytes(b.id) in used_ids:
            used_ids.remove(bytes(b.id))
            kept.append(b)
    kept.sort(key=_blob_order)
    return _coalesced(CopyPackBlobs.from_index_entry(index_pack.id, b) for b in kept)


class NewPack(NamedTuple):
    """A pack the copier wrote: ``data`` is a uint8 device tensor of exactly
    the pack file, ``id`` its SHA-256 (packer.rs:833, computed on the device),
    ``index`` the index.IndexPack that describes it."""
    id: bytes
    data: object
    index: IndexPack


@dataclass
class CopyStats:
    blobs_read: int = 0      # blobs taken out of source packs
    bytes_read: int = 0      # their sealed bytes
    blobs_skipped: int = 0   # blobs of the plan that were there already
    blobs_packed: int = 0    # blobs added to the packer (the open pack's included)
    bytes_packed: int = 0    # their sealed bytes


class _Txn:
    """The packer's state while one call runs; the copier takes it over only
    when the call has succeeded."""

    def __init__(self, c: "BlobCopier"):
        self.carry, self.carry_blobs = c._carry, c._carry_blobs
        self.sizer = _copy.copy(c.sizer)
        self.built: list = []        # (pack buffer, rcdc_pack array, blobs, offsets) per group
        self.closed_ids: set = set()
        self.stats = CopyStats()


_NO_BLOBS = np.zeros(0, PACK_BLOB)


class BlobCopier:
    """BlobCopier (packer.rs:908-1054) for packs in HBM.

    ``key_src`` / ``key_dst``: crypto.Key of the source and the destination
    (the same for prune).  ``blob_type`` (0 data, 1 tree) goes into every
    header entry (BlobCopier::new, :944-957).  ``indexer``: the destination's
    index.Indexer; every pack returned has been given to ``indexer.add``
    (FileWriterHandle::index, :784-791).  ``sizer``: PackSizer.fixed(..) for
    prune (prune.rs:1380-1382), PackSizer.from_config for copy
    (copy.rs:94-98); it grows by the size of every pack that closes.
    ``level``: the destination's config.zstd(), None to store blobs as they
    are.  ``nonces``: n -> (n, 16) uint8 array, pack.random_nonces by default;
    per call the copier draws one nonce per blob it seals, all at once and in
    plan order, and then the header nonces, one draw per group, in pack order.

    Packs close as RawPacker::add_raw / should_save close them
    (pack.group_blobs_open: MAX_COUNT blobs, or the size reaching
    sizer.pack_size()); the open pack's sealed blobs stay in a device buffer
    between calls, as in DeviceIngest._pack.  MAX_AGE, the wall-clock rule of
    should_save, is not modelled.  Everything runs on the current torch
    stream of the device; a call returns when its work is done.

    The blobs of the new packs are in the order of the plan.  The reference
    copies in parallel (copy.rs:167-169, prune.rs:1401-1403) and promises no
    order; this one promises the plan's.

    A call that raises has changed nothing: no pack, nothing in the indexer,
    nothing in the open pack, the sizer as it was.  Packs that earlier calls
    returned stand."""

    def __init__(self, key_src, key_dst, blob_type: int, indexer, sizer: PackSizer,
                 level: Optional[int], extra_verify: bool = True, device: int = 0,
                 batch_bytes: int = 1 << 30, nonces: Optional[Callable] = None):
        if blob_type not in (0, 1):
            raise RusticError(ErrorKind.InvalidInput, f"blob type {blob_type}")
        self.key_src, self.key_dst = key_src, key_dst
        self.blob_type = int(blob_type)
        self.indexer = indexer
        self.sizer = sizer
        self.level = level
        self.extra_verify = bool(extra_verify)
        self.device = int(device)
        self.batch_bytes = int(batch_bytes)
        self._nonces = nonces or random_nonces
        self.stats = CopyStats()
        self._carry = None              # sealed blobs of the open pack (device tensor)
        self._carry_blobs = _NO_BLOBS   # their rcdc_pack_blob rows, in_off into _carry

    @property
    def open_blobs(self) -> int:
        """Blobs of the open pack (added, not yet in a pack file)."""
        return len(self._carry_blobs)

    # ---- host helpers ------------------------------------------------------
    def _draw(self, n: int) -> np.ndarray:
        if n == 0:
            return np.zeros((0, 16), np.uint8)
        return np.asarray(self._nonces(n), np.uint8).reshape(n, 16)

    @staticmethod
    def _checked(pack_blobs: Sequence[CopyPackBlobs]) -> List[CopyPackBlobs]:
        """Every blob lies inside its read (the kernels take the offsets as
        they are)."""
        out = []
        for r in pack_blobs:
            for bl, bid in r.blobs:
                if (bl.offset < r.offset or bl.length < 0
                        or bl.offset + bl.length > r.offset + r.length or len(bytes(bid)) != 32):
                    raise RusticError(ErrorKind.InvalidInput,
                                      f"blob `{bytes(bid).hex()}` [{bl.offset}, +{bl.length}) is not "
                                      f"inside the read [{r.offset}, +{r.length}) of pack "
                                      f"`{bytes(r.pack_id).hex()}`")
            out.append(r)
        return out

    @staticmethod
    def _groups(reads, budget: int):
        """(read, kept blobs, bytes) in plan order in groups of at most
        ``budget`` bytes; a single read above the budget is a group of its
        own (restore._groups)."""
        groups, cur, size = [], [], 0
        for r, kept, n in reads:
            if cur and size + n > budget:
                groups.append(cur)
                cur, size = [], 0
            cur.append((r, kept))
            size += n
        if cur:
            groups.append(cur)
        return groups

    def _load(self, torch, dev, group, read_partial):
        """The reads of a group in one device buffer, 16-aligned, as
        restore_contents lays them; returns (buffer, offset per read)."""
        offs, total = [], 0
        for r, _ in group:
            offs.append(total)
            total = (total + r.length + 15) // 16 * 16
        raw = torch.empty(total + 64, dtype=torch.uint8, device=dev)
        host, tensors = None, []
        for (r, _), o in zip(group, offs):
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
        return raw, offs

    # ---- the packer ----------------------------------------------------------
    def _pack(self, torch, dev, s, t: _Txn, new_blobs: np.ndarray, src, finalize: bool) -> None:
        """Packer::add_raw for ``new_blobs`` (sealed, in the device tensor
        ``src``) after the open pack's: the packs should_save closes are built
        (rcdc_pack_build_raw_multi), the open pack's blobs move into a new
        carry buffer (rcdc_copy_ranges) -- the logic of DeviceIngest._pack."""
        from .crypto import _ctx
        ctx = _ctx(self.device)
        blobs = np.concatenate([t.carry_blobs, new_blobs])
        if not len(blobs):
            return
        grp, open_from = group_blobs_open(blobs["len"].astype(np.int64) - 32, t.sizer,
                                          blobs["uncompressed_len"], finalize)
        # source 0: the carry buffer, source 1: this group's sealed blobs
        ptrs = [x.data_ptr() for x in (t.carry, src) if x is not None]
        srcs = [ptrs[0], ptrs[-1]]
        if grp:
            closed = blobs[:open_from]
            packs_t, total = pack_layout(closed, grp, self._draw(len(grp)), align=256, raw=True)
            out = torch.empty(total + 64, dtype=torch.uint8, device=dev)
            offs = build_packs_multi(ctx, self.key_dst._key, srcs, closed, packs_t, out.data_ptr(),
                                     total, s)
            t.built.append((out[:total], packs_t, closed, offs))
            t.closed_ids.update(bytes(x) for x in closed["id"])
        rest = blobs[open_from:].copy()
        carry = None
        if len(rest):
            lens = rest["len"].astype(np.uint64)
            dst = np.zeros(len(rest), np.uint64)
            dst[1:] = np.cumsum((lens + 15) // 16 * 16)[:-1]
            carry = torch.empty(int(dst[-1] + lens[-1]) + 64, dtype=torch.uint8, device=dev)
            copy_ranges(ctx, srcs, rest["pad"], rest["in_off"], lens, dst, carry.data_ptr(), s)
            rest["in_off"] = dst
            rest["pad"] = 0
        t.carry, t.carry_blobs = carry, rest

    def _commit(self, torch, dev, t: _Txn) -> List[NewPack]:
        """The call has succeeded: its packs get their ids, the indexer gets
        their IndexPacks, the copier the new open pack.  A pack's SHA-256 is
        one serial chain (about a second per 32 MiB on the device), so the
        packs of all groups are hashed by one rcdc_sha256_chunks call, side by
        side: the groups' pack buffers are joined into one for it (a device
        copy of the call's output, which then takes the buffers' place)."""
        from .crypto import _ctx
        from .device import sha256_device
        out: List[NewPack] = []
        if t.built:
            bufs = [b[0] for b in t.built]
            arena = bufs[0] if len(bufs) == 1 else torch.cat(bufs)
            del bufs
            rows, base = [], 0
            for buf, packs_t, _, _ in t.built:
                rows += [[base + int(p["out_off"]), int(p["size"])] for p in packs_t]
                base += int(buf.numel())
            refs = torch.tensor(rows, dtype=torch.int64, device=dev).reshape(-1, 2)
            dig = sha256_device(_ctx(self.device), arena, refs)
            torch.cuda.synchronize(dev)
            ids = dig.cpu().numpy()
            now = rustic_time()
            for _, packs_t, closed, offs in t.built:
                plain = closed.copy()
                plain["len"] -= 32   # index_entries adds the sealing to the length
                for k, entries in enumerate(index_entries(plain, packs_t, offs)):
                    ip = IndexPack(ids[len(out)].tobytes(), time=now)
                    for e in entries:
                        ip.add(*e)
                    o, n = rows[len(out)]
                    out.append(NewPack(ip.id, arena[o:o + n], ip))
            t.built = []
        else:
            torch.cuda.synchronize(dev)
        self._carry, self._carry_blobs = t.carry, t.carry_blobs
        self.sizer.current_size = t.sizer.current_size
        for f in ("blobs_read", "bytes_read", "blobs_skipped", "blobs_packed", "bytes_packed"):
            setattr(self.stats, f, getattr(self.stats, f) + getattr(t.stats, f))
        for p in out:
            self.indexer.add(p.index)
        return out

    def _new_blobs(self, in_offs, sealed_lens, ids, ulens) -> np.ndarray:
        n = len(ids)
        b = make_blobs(in_offs, sealed_lens, np.frombuffer(b"".join(ids), np.uint8).reshape(n, 32),
                       np.zeros((n, 16), np.uint8), types=[self.blob_type] * n, uncompressed=ulens)
        b["pad"] = 1
        return b

    # ---- the copies ----------------------------------------------------------
    def copy(self, pack_blobs: Sequence[CopyPackBlobs], read_partial: Callable,
             progress: Optional[Callable] = None) -> List[NewPack]:
        """BlobCopier::copy (packer.rs:1017-1048) for a list of CopyPackBlobs,
        taken in list order.  ``read_partial(pack_id, offset, length)`` returns
        exactly ``length`` bytes of that pack (bytes or a uint8 device tensor),
        as for restore_contents.  Returns the packs that closed.

        A blob is skipped when ``indexer.has(id)`` holds or the id is in the
        open pack already (packer.rs:264-266) -- from earlier in this call or
        from an earlier call.  One difference from the reference: a skipped
        blob is not opened or decoded, and a read none of whose blobs is
        needed is not made; the reference reads them and drops them
        (restore_contents makes the same choice).

        The reads that are left are taken in groups of at most ``batch_bytes``
        decoded bytes (a single read above that is a group of its own).  Per
        group the read_partial results are laid into one device buffer, one
        read_blobs(key_src) call opens and decodes the blobs, one
        process_blobs(key_dst) call compresses at ``level``, seals and (with
        ``extra_verify``) verifies them, and the packer builds the packs that
        close, so the number of device calls grows with the groups, not with
        the blobs; only statuses, lengths and pack ids go to the host.

        Errors of read_blobs (MAC, decode, length) and of process_blobs
        (verification, u32 length) propagate as they are.  ``progress`` is
        called with ``blob.length`` for every blob of the plan, copied or
        skipped (``p.inc``: the reference's total counts them all)."""
        import torch
        from .compress import process_blobs
        from .read import read_blobs
        dev = torch.device("cuda", self.device)
        t = _Txn(self)
        seen = {bytes(x) for x in t.carry_blobs["id"]}
        reads = []
        for r in self._checked(pack_blobs):
            kept = []
            for bl, bid in r.blobs:
                bid = bytes(bid)
                if self.indexer.has(bid) or bid in seen:
                    t.stats.blobs_skipped += 1
                    if progress is not None:
                        progress(bl.length)
                else:
                    seen.add(bid)
                    kept.append((bl, bid))
            if kept:
                reads.append((r, kept, sum(data_length(bl) for bl, _ in kept)))
        nonces = self._draw(sum(len(kept) for _, kept, _ in reads))
        done = 0
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev).cuda_stream
            for group in self._groups(reads, self.batch_bytes):
                raw, offs = self._load(torch, dev, group, read_partial)
                entries = [IndexBlob(bid, self.blob_type, o + bl.offset - r.offset, bl.length,
                                     bl.uncompressed_length or None)
                           for (r, kept), o in zip(group, offs) for bl, bid in kept]
                n = len(entries)
                plain = read_blobs(self.key_src, raw, entries, self.device)
                del raw
                sealed, s_offs, s_lens, _, ulens = process_blobs(
                    self.key_dst, plain.data.data_ptr(), plain.offsets, plain.lengths, self.level,
                    nonces[done:done + n], self.device, self.extra_verify)
                del plain
                done += n
                self._pack(torch, dev, s, t,
                           self._new_blobs(s_offs, s_lens, [e.id for e in entries], ulens), sealed,
                           False)
                t.stats.blobs_read += n
                t.stats.bytes_read += sum(int(e.length) for e in entries)
                t.stats.blobs_packed += n
                t.stats.bytes_packed += int(np.asarray(s_lens, np.uint64).sum())
                if progress is not None:
                    for e in entries:
                        progress(e.length)
            return self._commit(torch, dev, t)

    def copy_fast(self, pack_blobs: Sequence[CopyPackBlobs], read_partial: Callable,
                  progress: Optional[Callable] = None) -> List[NewPack]:
        """BlobCopier::copy_fast (packer.rs:970-1004): the sealed bytes of
        each blob go into the new packs exactly as they are, with their
        ``uncompressed_length``; nothing is opened, so it serves only where
        source and destination share key and format.  A blob is skipped only
        when ``indexer.has(id)`` holds (Packer::add_raw, :331-347) -- which
        covers the packs this call has closed so far; an id that is only in
        the open pack is written again.  (The reference's BasicPacker::add_raw
        looks into the open pack once more, :622; that second look is not
        modelled.)  Reads none of whose blobs is needed are not made.  Groups
        are of at most ``batch_bytes`` sealed bytes; errors, ``progress`` and
        the all-or-nothing rule are copy's."""
        import torch
        dev = torch.device("cuda", self.device)
        t = _Txn(self)
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev).cuda_stream
            reads = [(r, r.blobs, sum(int(bl.length) for bl, _ in r.blobs))
                     for r in self._checked(pack_blobs)]
            for group in self._groups(reads, self.batch_bytes):
                # what the packs closed by the groups before hold is in the
                # indexer by now, as far as add_raw can tell
                kept_group = []
                for r, blobs in group:
                    kept = []
                    for bl, bid in blobs:
                        bid = bytes(bid)
                        if self.indexer.has(bid) or bid in t.closed_ids:
                            t.stats.blobs_skipped += 1
                        else:
                            kept.append((bl, bid))
                    if kept:
                        kept_group.append((r, kept))
                if kept_group:
                    raw, offs = self._load(torch, dev, kept_group, read_partial)
                    rows = [(o + bl.offset - r.offset, bl.length, bid, bl.uncompressed_length)
                            for (r, kept), o in zip(kept_group, offs) for bl, bid in kept]
                    self._pack(torch, dev, s, t,
                               self._new_blobs([x[0] for x in rows], [x[1] for x in rows],
                                               [x[2] for x in rows], [x[3] for x in rows]),
                               raw, False)
                    del raw
                    t.stats.blobs_read += len(rows)
                    t.stats.bytes_read += sum(x[1] for x in rows)
                    t.stats.blobs_packed += len(rows)
                    t.stats.bytes_packed += sum(x[1] for x in rows)
                if progress is not None:
                    for r, blobs in group:
                        for bl, _ in blobs:
                            progress(bl.length)
            return self._commit(torch, dev, t)

    def finalize(self) -> List[NewPack]:
        """Packer::finalize (packer.rs:354-361, :456-464): the open pack, if
        it holds a blob, is closed and returned.  The copier can go on
        afterwards."""
        import torch
        dev = torch.device("cuda", self.device)
        t = _Txn(self)
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev).cuda_stream
            self._pack(torch, dev, s, t, _NO_BLOBS, None, True)
            return self._commit(torch, dev, t)
