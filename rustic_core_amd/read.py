"""The read direction on the device: sealed blobs of a pack in HBM opened,
decompressed and checked (rcdc_aead_open, rcdc_zstd_decompress,
rcdc_sha256_chunks in include/rcdc.h).

Reference: ``DecryptReadBackend::read_encrypted_from_partial``
(crates/core/src/backend/decrypt.rs:71-97) -- what ``restore``, ``copy`` and
``prune``'s repack read blobs with -- and ``check_pack``
(commands/check.rs:718-814) of ``check --read-data``.  ``read_blobs`` is the
first for a batch of blobs of one pack; ``check_pack`` follows the second
step by step.  No CPU fallback.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from .compress import DEC_OK, DECODE_MESSAGE, decompress_frames
from .crypto import Key, _ctx, make_refs as aead_refs
from .errors import ErrorKind, RusticError
from .pack import header_size, parse_header

MAC_MESSAGE = "Data decryption failed, MAC check failed."  # aespoly1305.rs:97-108
SHORT_MESSAGE = "Data is too short (less than 16 bytes), cannot decrypt."  # :89-94


def _ulen(e) -> int:
    """An entry's uncompressed length, 0 when stored (pack.HeaderBlob's
    ``uncompressed_len`` / index.IndexBlob's ``uncompressed_length``)."""
    return int(getattr(e, "uncompressed_len", None) or getattr(e, "uncompressed_length", None) or 0)


def _length_message(actual: int, expected: int) -> str:  # decrypt.rs:86-93
    return (f"Length of uncompressed data `{actual}` does not match the given length "
            f"`{expected}`.")


class PlainBlobs(NamedTuple):
    """read_blobs' result: blob i is data[offsets[i] : offsets[i] + lengths[i]]."""
    data: object  # uint8 device tensor
    offsets: np.ndarray
    lengths: np.ndarray


def _open(key: Key, d_pack, entries, ctx, stream):
    """Every entry's sealed bytes opened into one device tensor (16-aligned
    plaintexts); raises what Key.decrypt_data raises."""
    import torch
    n = len(entries)
    lens = np.array([int(e.length) for e in entries], np.int64)
    if n and int(lens.min()) < 16:
        raise RusticError(ErrorKind.Cryptography, SHORT_MESSAGE)
    plain = np.maximum(lens - 32, 0)
    p_offs = np.zeros(n, np.uint64)
    o = 0
    for i in range(n):
        p_offs[i] = o
        o = (o + int(plain[i]) + 15) // 16 * 16
    buf = torch.empty(o + 64, dtype=torch.uint8, device=d_pack.device)
    if n:
        st = key.open_blobs(d_pack.data_ptr(), aead_refs([int(e.offset) for e in entries], lens, p_offs),
                            buf.data_ptr(), stream, ctx)
        if st.any():
            raise RusticError(ErrorKind.Cryptography, MAC_MESSAGE)
    return buf, p_offs, plain.astype(np.uint64)


def _decode(ctx, buf, p_offs, p_lens, ulens, stream, exact: bool):
    """The opened blobs that have an uncompressed length decoded with that
    capacity; the others left where they are.  Returns (tensor, offsets,
    lengths, decoder status, decoded lengths) over all blobs.  ``exact``:
    read_encrypted_from_partial's errors; otherwise only the decode error."""
    import torch
    n = len(ulens)
    comp = [i for i in range(n) if ulens[i]]
    offs, lens = p_offs.copy(), p_lens.copy()
    dst = np.zeros(n, np.uint32)
    dlen = p_lens.copy()
    if not comp:
        return buf, offs, lens, dst, dlen
    o_offs, o = [], 0
    for i in comp:
        o_offs.append(o)
        o = (o + int(ulens[i]) + 15) // 16 * 16
    out = torch.empty(int(buf.numel()) + o + 64, dtype=torch.uint8, device=buf.device)
    base = int(buf.numel())
    out[:base] = buf  # the stored blobs stay at their offsets
    st, ln = decompress_frames(ctx, buf.data_ptr(), [int(p_offs[i]) for i in comp],
                               [int(p_lens[i]) for i in comp], out.data_ptr(),
                               [base + x for x in o_offs], [int(ulens[i]) for i in comp], stream)
    for k, i in enumerate(comp):
        dst[i], dlen[i] = st[k], ln[k]
        offs[i], lens[i] = base + o_offs[k], ln[k]
        if int(st[k]) == 2:
            raise RusticError(ErrorKind.Internal, DECODE_MESSAGE)
        if exact and (int(st[k]) != DEC_OK or int(ln[k]) != int(ulens[i])):
            actual = f"more than {int(ulens[i])}" if int(st[k]) != DEC_OK else str(int(ln[k]))
            raise RusticError(ErrorKind.Internal, _length_message(actual, int(ulens[i])))
    # check_pack: the reference decodes whatever the frame holds and then
    # compares lengths, so a frame that does not fit the indexed length is
    # decoded again with room (doubling, from one block more)
    retry = [i for i in comp if int(dst[i]) == 1]
    cap = 0
    while retry and not exact:
        cap = max(2 * cap, 2 * max(int(ulens[i]) for i in retry) + (128 << 10))
        if cap > 1 << 32:
            raise RusticError(ErrorKind.Internal, DECODE_MESSAGE)
        extra = torch.empty(len(retry) * cap + 64, dtype=torch.uint8, device=buf.device)
        st, ln = decompress_frames(ctx, buf.data_ptr(), [int(p_offs[i]) for i in retry],
                                   [int(p_lens[i]) for i in retry], extra.data_ptr(),
                                   [k * cap for k in range(len(retry))], [cap] * len(retry), stream)
        if (st == 2).any():
            raise RusticError(ErrorKind.Internal, DECODE_MESSAGE)
        if (st == 0).all():
            base2 = int(out.numel())
            out = torch.cat([out, extra])
            for k, i in enumerate(retry):
                dst[i], dlen[i] = 0, ln[k]
                offs[i], lens[i] = base2 + k * cap, ln[k]
            retry = []
    return out, offs, lens, dst, dlen


def read_blobs(key: Key, d_pack, entries: Sequence, device: int = 0) -> PlainBlobs:
    """read_encrypted_from_partial (decrypt.rs:71-97) for a batch: ``entries``
    (pack.HeaderBlob or index.IndexBlob: offset, length, uncompressed length
    or none) locate sealed blobs in the uint8 device tensor ``d_pack``.  Every
    blob is opened (a failed MAC raises what Key.decrypt_data raises); the
    ones with an uncompressed length are decompressed with exactly that
    capacity.  A frame that does not decode raises ErrorKind.Internal "Failed
    to decode zstd compressed data ..."; one that decodes to another length
    (or does not fit the given one) raises ErrorKind.Internal "Length of
    uncompressed data ... does not match the given length ...".  Returns the
    plain blobs in one device tensor with their offsets and lengths."""
    import torch
    ctx = _ctx(device)
    with torch.cuda.device(d_pack.device):
        s = torch.cuda.current_stream(d_pack.device).cuda_stream
        buf, p_offs, p_lens = _open(key, d_pack, entries, ctx, s)
        ulens = [_ulen(e) for e in entries]
        out, offs, lens, _, _ = _decode(ctx, buf, p_offs, p_lens, ulens, s, exact=True)
    return PlainBlobs(out, offs, lens)


class Finding(NamedTuple):
    """One CheckError (check.rs:816-): its variant's name and fields."""
    kind: str
    fields: dict


def _sha256(ctx, tensor, offs, lens) -> List[bytes]:
    import torch
    from .device import sha256_device
    refs = torch.tensor([[int(o), int(n)] for o, n in zip(offs, lens)], dtype=torch.int64,
                        device=tensor.device).reshape(-1, 2)
    dig = sha256_device(ctx, tensor, refs)
    torch.cuda.synchronize(tensor.device)
    h = dig.cpu().numpy()
    return [h[i].tobytes() for i in range(len(lens))]


def check_pack(key: Key, index_pack, pack, device: int = 0) -> List[Finding]:
    """check_pack (check.rs:718-814) for one pack: ``index_pack`` is the
    index.IndexPack that describes it, ``pack`` its bytes (bytes or a uint8
    device tensor).  The steps and their early returns are the reference's:

    1. PackSizeMismatch: the bytes' length against IndexPack.pack_size();
    2. PackHashMismatch: the pack id against the SHA-256 of the whole pack
       (on the device);
    3. PackHeaderLengthMismatch: pack.header_size(index blobs) + 32 against
       the trailing u32;
    4. the header opened and parsed (pack.parse_header); any difference from
       the sorted index blobs is PackHeaderMismatchIndex;
    5. per blob, in that order: opened, decompressed when the index gives an
       uncompressed length, then PackBlobLengthMismatch and
       PackBlobHashMismatch (SHA-256 of the decoded bytes on the device).

    Steps 1-4 return at their finding; step 5 collects.  A MAC that does not
    verify raises (``be.decrypt(..)?``).  One difference from the reference: a
    frame that does not decode is a panic there (``decode_all(..).unwrap()``,
    check.rs:796); here it raises the decode_all error (ErrorKind.Internal,
    "Failed to decode zstd compressed data ...")."""
    import torch
    ctx = _ctx(device)
    dev = torch.device("cuda", device)
    n = pack.numel() if hasattr(pack, "numel") else len(pack)
    pid = bytes(index_pack.id)
    size = int(index_pack.pack_size())
    if n != size:
        return [Finding("PackSizeMismatch", dict(id=pid, size=int(n), expected=size))]
    if hasattr(pack, "numel"):
        d_pack = pack
    else:
        host = torch.zeros(n + 4, dtype=torch.uint8)
        if n:
            host[:n] = torch.frombuffer(bytearray(pack), dtype=torch.uint8)
        d_pack = host.to(dev)
    with torch.cuda.device(d_pack.device):
        s = torch.cuda.current_stream(d_pack.device).cuda_stream
        comp_id = _sha256(ctx, d_pack, [0], [n])[0]
        if comp_id != pid:
            return [Finding("PackHashMismatch", dict(id=pid, comp_id=comp_id))]
        header_len = header_size(index_pack.blobs) + 32
        if n < 4:
            raise RusticError(ErrorKind.Internal,
                              f"Error reading pack header length `{header_len}` for `{pid.hex()}`")
        pack_header_len = int.from_bytes(d_pack[n - 4:n].cpu().numpy().tobytes(), "little")
        if pack_header_len != header_len:
            return [Finding("PackHeaderLengthMismatch",
                            dict(id=pid, length=pack_header_len, computed=header_len))]

        class _Hdr(NamedTuple):
            offset: int
            length: int

        hbuf, hoffs, hlens = _open(key, d_pack, [_Hdr(n - 4 - header_len, header_len)], ctx, s)
        torch.cuda.synchronize(d_pack.device)
        header = hbuf[:int(hlens[0])].cpu().numpy().tobytes()
        pack_blobs = [(b.id, b.type, b.offset, b.length, b.uncompressed_len or None)
                      for b in parse_header(header)]
        # IndexBlob's order (indexfile.rs: by BlobLocation, offset first)
        blobs = sorted(index_pack.blobs, key=lambda b: (b.offset, b.length, _ulen(b), b.type, b.id))
        if pack_blobs != [(bytes(b.id), b.type, b.offset, b.length, _ulen(b) or None) for b in blobs]:
            return [Finding("PackHeaderMismatchIndex", dict(id=pid))]
        # the blobs: the reference reads them one after another from the front
        # (data.split_to(length)), which is where the header's offsets point
        findings: List[Finding] = []
        buf, p_offs, p_lens = _open(key, d_pack, blobs, ctx, s)
        ulens = [_ulen(b) for b in blobs]
        out, offs, lens, dst, dlen = _decode(ctx, buf, p_offs, p_lens, ulens, s, exact=False)
        # a frame longer than the index says did not fit (status 1): its length
        # differs, and so does the hash of what would have been decoded
        ids = _sha256(ctx, out, offs, lens) if len(blobs) else []
        for i, b in enumerate(blobs):
            if ulens[i] and (int(dst[i]) != DEC_OK or int(dlen[i]) != ulens[i]):
                findings.append(Finding("PackBlobLengthMismatch", dict(id=pid, blob_id=bytes(b.id))))
            if int(dst[i]) != DEC_OK or ids[i] != bytes(b.id):
                findings.append(Finding("PackBlobHashMismatch",
                                        dict(id=pid, blob_id=bytes(b.id),
                                             comp_id=ids[i] if int(dst[i]) == DEC_OK else None)))
    return findings
