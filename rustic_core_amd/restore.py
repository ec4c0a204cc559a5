"""Restore of file contents on the device: the plan, the reads and the byte
work of ``restore`` for packs and files in HBM (rcdc_place_blobs in
include/rcdc.h, after read.read_blobs).

Reference: ``commands/restore.rs`` -- ``RestorePlan::add_file`` (:744-837)
decides which blobs of which packs go to which positions of which files,
with ``blob_matches_reader`` (id.rs:200-204) over a file that is already at
the destination; ``restore_contents`` (:530-677) reads every needed part of
every pack once (``PackInfo::coalesce`` :494-508 over
``BlobLocations::can_coalesce`` / ``append``, blob.rs:185-196), opens and
decodes each blob (``read_encrypted_from_partial``) and writes it to every
file position that holds it, skipping all-zero blobs under
``SparseRestore::ByContent``.  Metadata, directories, links, the mtime
shortcut and writing to disk stay with the caller.  No CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .errors import ErrorKind, RusticError
from .index import IndexBlob

MAX_HOLESIZE = 256 << 10     # blob.rs:17
LIMIT_PACK_READ = 40 << 20   # blob.rs:15


def index_lookup(index_files) -> Dict[bytes, Tuple[bytes, IndexBlob]]:
    """Blob id -> (pack id, IndexBlob) over the ``packs`` of index.IndexFiles
    (``packs_to_delete`` is ignored); the first entry of an id wins."""
    out: Dict[bytes, Tuple[bytes, IndexBlob]] = {}
    for f in index_files:
        for p in f.packs:
            for b in p.blobs:
                out.setdefault(bytes(b.id), (bytes(p.id), b))
    return out


def _entry(index, blob_id: bytes) -> Tuple[bytes, IndexBlob]:
    """Repository::get_index_entry (repository.rs:1347-1359)."""
    e = index.get(bytes(blob_id))
    if e is None:
        raise RusticError(ErrorKind.Internal,
                          f"Blob ID `{bytes(blob_id).hex()}` not found in index, but should be there.")
    return e


def _entries(index, content_ids) -> List[Tuple[bytes, IndexBlob]]:
    """_entry per content id; a DeviceIndex answers them in one device call."""
    from .dindex import DATA, DeviceIndex
    if not isinstance(index, DeviceIndex):
        return [_entry(index, i) for i in content_ids]
    content_ids = [bytes(i) for i in content_ids]
    found = index.entries(DATA, content_ids)
    return [_entry({i: e}, i) for i, e in zip(content_ids, found)]


def data_length(b) -> int:
    """BlobLocation::data_length (blob.rs:146-151): the uncompressed length,
    or the sealed length less the 32 bytes of sealing."""
    ul = getattr(b, "uncompressed_length", None)
    return int(ul) if ul else int(b.length) - 32


class BlobLocation(NamedTuple):
    """blob.rs BlobLocation; ``uncompressed_length`` 0 stands for None."""
    offset: int
    length: int
    uncompressed_length: int = 0


class FileLocation(NamedTuple):
    """restore.rs:706-715."""
    file_idx: int
    file_start: int
    matches: bool


class PackRead(NamedTuple):
    """restore.rs PackInfo with its BlobLocations flattened: one read of
    ``length`` bytes at ``offset`` of pack ``pack_id`` -- or, with
    ``from_file`` = (file_idx, file_start, data_length), of a file that holds
    the blob already.  ``blobs``: [(BlobLocation, [(file_idx, file_start)])],
    the destinations being the positions that do not match."""
    pack_id: bytes
    from_file: Optional[Tuple[int, int, int]]
    offset: int
    length: int
    blobs: list


def can_coalesce(offset: int, length: int, other_offset: int, other_length: int) -> bool:
    """BlobLocations::can_coalesce (blob.rs:185-190)."""
    return (other_offset <= offset + length + MAX_HOLESIZE
            and other_offset >= offset + length
            and other_offset + other_length - offset <= LIMIT_PACK_READ)


def coalesce(a: PackRead, b: PackRead) -> Optional[PackRead]:
    """PackInfo::coalesce (restore.rs:494-508): the merged read, or None.  The
    left read's ``from_file`` (None) is kept, the right one's is dropped, as
    ``append`` does there."""
    if (a.pack_id == b.pack_id and a.from_file is None
            and can_coalesce(a.offset, a.length, b.offset, b.length)):
        return PackRead(a.pack_id, a.from_file, a.offset, b.offset + b.length - a.offset,
                        a.blobs + b.blobs)
    return None


def _as_device(x, dev):
    """bytes -> a uint8 device tensor (tensors pass through)."""
    import torch
    if hasattr(x, "data_ptr"):
        return x
    n = len(x)
    host = torch.zeros(n + 4, dtype=torch.uint8)  # frombuffer refuses an empty buffer
    if n:
        host[:n] = torch.frombuffer(bytearray(x), dtype=torch.uint8)
    return host.to(dev)[:n]


class RestorePlan:
    """restore.rs:687-702: ``names``, ``file_lengths``, the restore info
    ``r`` {(pack id, offset, length, uncompressed_length or 0):
    [FileLocation]}, ``restore_size`` and ``matched_size``.  ``existing``
    keeps the device tensor of every registered file that was given one of
    the right size (what restore_contents writes in place)."""

    def __init__(self):
        self.names: list = []
        self.file_lengths: List[int] = []
        self.r: Dict[Tuple[bytes, int, int, int], List[FileLocation]] = {}
        self.restore_size = 0
        self.matched_size = 0
        self.existing: Dict[int, object] = {}

    def restore_info(self):
        """The entries in BTreeMap<(PackId, BlobLocation), _> order: pack id
        bytes, then offset, length, uncompressed length (None first)."""
        return sorted(self.r.items(), key=lambda kv: kv[0])

    def add_file(self, name, size: int, content_ids: Sequence[bytes], index, existing=None,
                 device: int = 0) -> str:
        """RestorePlan::add_file (restore.rs:744-837) without the mtime
        branch.  ``existing``: the file already at the destination (uint8
        device tensor, or bytes, which are uploaded); it counts only when its
        length is ``size`` (get_matching_file).  ``index``: index_lookup's
        dict, or a ``dindex.DeviceIndex`` over the same index files (one
        ``entries`` call per file).  Whether each blob is already in place (blob_matches_reader) is
        one sha256_device call over the ranges [file_pos, file_pos +
        data_length) of ``existing``.  Returns "Existing", "Verified" or
        "Modify"."""
        import torch
        n_exist = None if existing is None else (
            int(existing.numel()) if hasattr(existing, "numel") else len(existing))
        open_file = existing if n_exist is not None and n_exist == int(size) else None
        if int(size) == 0 and open_file is not None:
            return "Existing"  # an empty file of the right size
        entries = _entries(index, content_ids)
        lens = [data_length(b) for _, b in entries]
        pos = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)
        matches = [False] * len(entries)
        if open_file is not None and entries:
            from .crypto import _ctx
            from .device import sha256_device
            dev = torch.device("cuda", device)
            open_file = _as_device(open_file, dev)
            # a range past the end of the file cannot match (the reader comes
            # up short); an empty blob matches by its id alone
            import hashlib
            which = [i for i in range(len(entries)) if lens[i] and pos[i] + lens[i] <= n_exist]
            for i in range(len(entries)):
                if not lens[i]:
                    matches[i] = bytes(content_ids[i]) == hashlib.sha256(b"").digest()
            if which:
                with torch.cuda.device(dev):
                    refs = torch.tensor([[int(pos[i]), lens[i]] for i in which], dtype=torch.int64,
                                        device=dev).reshape(-1, 2)
                    dig = sha256_device(_ctx(device), open_file, refs)
                    torch.cuda.synchronize(dev)
                    h = dig.cpu().numpy()
                for k, i in enumerate(which):
                    matches[i] = h[k].tobytes() == bytes(content_ids[i])
        file_idx = len(self.names)
        self.names.append(name)
        has_unmatched = False
        for i, (pack_id, b) in enumerate(entries):
            key = (pack_id, int(b.offset), int(b.length), int(b.uncompressed_length or 0))
            self.r.setdefault(key, []).append(FileLocation(file_idx, int(pos[i]), matches[i]))
            if matches[i]:
                self.matched_size += lens[i]
            else:
                self.restore_size += lens[i]
                has_unmatched = True
        self.file_lengths.append(int(pos[-1]))
        if open_file is not None:
            self.existing[file_idx] = open_file
        return "Verified" if not has_unmatched and open_file is not None else "Modify"

    def pack_reads(self) -> List[PackRead]:
        """The ``packs`` vector of restore_contents (restore.rs:561-583): one
        PackRead per entry of the restore info, ``from_file`` its first
        matching location, then neighbours coalesced."""
        out: List[PackRead] = []
        for (pack_id, off, ln, ul), fls in self.restore_info():
            bl = BlobLocation(off, ln, ul)
            from_file = next(((f.file_idx, f.file_start, data_length(bl)) for f in fls if f.matches),
                             None)
            dests = [(f.file_idx, f.file_start) for f in fls if not f.matches]
            cur = PackRead(pack_id, from_file, off, ln, [(bl, dests)])
            merged = coalesce(out[-1], cur) if out else None
            if merged is not None:
                out[-1] = merged
            else:
                out.append(cur)
        return out

    def to_packs(self) -> List[bytes]:
        """restore.rs:843-851: the packs of the entries none of whose
        locations match, neighbours deduplicated."""
        out: List[bytes] = []
        for (pack_id, _, _, _), fls in self.restore_info():
            if all(not f.matches for f in fls) and (not out or out[-1] != pack_id):
                out.append(pack_id)
        return out


class Restored(NamedTuple):
    files: list          # uint8 device tensor per file of the plan
    holes: list          # sorted (file_idx, start, length) of the skipped destinations
    zero_blobs: int      # placed blobs whose every byte is 0


def from_packs(mapping) -> Callable:
    """A ``read_partial`` over whole packs: {pack id: bytes or uint8 device
    tensor}."""
    def read_partial(pack_id, offset, length):
        return mapping[bytes(pack_id)][offset:offset + length]
    return read_partial


def _groups(reads: List[PackRead], budget: int) -> List[List[PackRead]]:
    """Reads in plan order in groups of at most ``budget`` decoded bytes; a
    single read above the budget is a group of its own."""
    groups, cur, size = [], [], 0
    for r in reads:
        n = sum(data_length(bl) for bl, dests in r.blobs if dests)
        if cur and size + n > budget:
            groups.append(cur)
            cur, size = [], 0
        cur.append(r)
        size += n
    if cur:
        groups.append(cur)
    return groups


def restore_contents(key, plan: RestorePlan, read_partial: Callable, existing=None,
                     sparse: bool = False, batch_bytes: int = 1 << 30,
                     device: int = 0) -> Restored:
    """restore_contents (restore.rs:530-677) into device tensors.

    ``read_partial(pack_id, offset, length)`` returns exactly ``length`` bytes
    of that pack (bytes or a uint8 device tensor): ``be.read_partial(
    FileType::Pack, ..)``.  ``files[i]`` is a uint8 device tensor of
    ``plan.file_lengths[i]`` bytes: the ``existing`` tensor of file i itself,
    written in place, when one of the right size is there (``existing`` maps
    file index to tensor; None: the tensors the plan kept from add_file),
    otherwise a new zero tensor.

    The reads of plan.pack_reads() are taken in order, in groups of at most
    ``batch_bytes`` decoded bytes.  Per group the read_partial results are laid
    into one device buffer, one read_blobs call opens and decodes every blob
    that has a destination, and one place_blobs call (rcdc_place_blobs)
    scatters them -- and the blobs a ``from_file`` read takes out of
    ``files[file_idx]`` -- into the file tensors, so the number of device
    calls grows with the groups, not with the blobs.  With ``sparse``
    (SparseRestore::ByContent) all-zero blobs are not written and ``holes``
    lists their destinations; ``zero_blobs`` counts them either way.

    Two differences from the reference.  An existing file of another size
    starts from zeros here; the reference's set_len keeps its old bytes under
    the blobs a sparse restore skips.  And a blob with no destination left
    (every position matched) is not read, opened or decoded; the reference
    reads it and drops it.

    Errors of read_blobs (MAC, decode, length) propagate as they are -- the
    reference panics there (unwrap, restore.rs:624-643) -- and leave the file
    tensors unspecified.  Everything runs on the current torch stream of the
    device."""
    import torch
    from .crypto import _ctx
    from .pack import PLACE_BLOB, PLACE_DEST, place_blobs
    from .read import read_blobs
    dev = torch.device("cuda", device)
    ctx = _ctx(device)
    if existing is None:
        existing = plan.existing
    holes: list = []
    zero_blobs = 0
    with torch.cuda.device(dev):
        files = []
        for i, n in enumerate(plan.file_lengths):
            e = existing.get(i) if existing else None
            if e is not None and hasattr(e, "data_ptr") and int(e.numel()) == n:
                files.append(e)
            else:
                files.append(torch.zeros(n, dtype=torch.uint8, device=dev))
        reads = [r for r in plan.pack_reads() if any(dests for _, dests in r.blobs)]
        for group in _groups(reads, int(batch_bytes)):
            # 1. the pack parts of the group in one device buffer, 16-aligned
            parts, total = [], 0
            for r in group:
                if r.from_file is None:
                    parts.append((r, total))
                    total = (total + r.length + 15) // 16 * 16
            raw = torch.empty(total + 64, dtype=torch.uint8, device=dev)
            host = None
            tensors = []
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
            # 2. every blob that has a destination, opened and decoded
            entries, owners = [], []
            for r, o in parts:
                for bl, dests in r.blobs:
                    if dests:
                        entries.append(IndexBlob(b"", 0, o + bl.offset - r.offset, bl.length,
                                                 bl.uncompressed_length or None))
                        owners.append((bl, dests))
            plain = read_blobs(key, raw, entries, device) if entries else None
            # 3. one scatter: the decoded buffer and the files that serve
            # from_file reads are the sources
            srcs = [plain.data] if plain is not None else []
            src_of: Dict[int, int] = {}
            out_of: Dict[int, int] = {}
            outs: list = []
            rows, drows = [], []

            def add(in_off, n, src, dests):
                for fi, start in dests:
                    if fi not in out_of:
                        out_of[fi] = len(outs)
                        outs.append(files[fi])
                    drows.append((start, out_of[fi]))
                rows.append((in_off, n, src, len(drows) - len(dests), len(dests), dests))

            for k, (bl, dests) in enumerate(owners):
                add(int(plain.offsets[k]), int(plain.lengths[k]), 0, dests)
            for r in group:
                if r.from_file is not None:
                    fi, start, n = r.from_file
                    if fi not in src_of:
                        src_of[fi] = len(srcs)
                        srcs.append(files[fi])
                    for bl, dests in r.blobs:
                        if dests:
                            add(start, n, src_of[fi], dests)
            if not rows:
                continue
            blobs = np.zeros(len(rows), PLACE_BLOB)
            blobs["in_off"] = [x[0] for x in rows]
            blobs["len"] = [x[1] for x in rows]
            blobs["src"] = [x[2] for x in rows]
            blobs["dest0"] = [x[3] for x in rows]
            blobs["ndests"] = [x[4] for x in rows]
            dd = np.zeros(len(drows), PLACE_DEST)
            dd["out_off"] = [x[0] for x in drows]
            dd["dst"] = [x[1] for x in drows]
            zero = place_blobs(ctx, [t.data_ptr() for t in srcs], [int(t.numel()) for t in srcs],
                               blobs, dd, [t.data_ptr() for t in outs],
                               [int(t.numel()) for t in outs], skip_zero=bool(sparse),
                               stream=torch.cuda.current_stream(dev).cuda_stream)
            zero_blobs += int(zero.sum())
            if sparse:
                for z, x in zip(zero, rows):
                    if z:
                        holes.extend((fi, start, x[1]) for fi, start in x[5])
    return Restored(files, sorted(holes), zero_blobs)
