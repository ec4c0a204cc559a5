"""The read direction on the device (rustic_core_amd/read.py): read_blobs is
read_encrypted_from_partial (crates/core/src/backend/decrypt.rs:71-97) for a
batch, check_pack follows commands/check.rs:718-814.  Against the reference's
own pack file (tests/golden, repo_mixed) and packs built on the device."""
import hashlib

import numpy as np
import pytest

from oracle import oracle, zstd_ref as zr
from tests.test_gpu_pack import _build
from tests.test_gpu_zstd_check import _data, _device_frames
from tests.test_pack_oracle import reference_pack

pytestmark = pytest.mark.gpu


def _dev(b: bytes):
    import torch
    t = torch.zeros(len(b) + 4, dtype=torch.uint8)
    t[:len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
    return t.to("cuda:0")[:len(b)]


def _index_pack(pack: bytes, entries, pid=None):
    from rustic_core_amd.index import IndexPack
    ip = IndexPack(hashlib.sha256(pack).digest() if pid is None else pid)
    for e in entries:
        ip.add(e.id, e.type, e.offset, e.length, e.uncompressed_len or None)
    return ip


def _plain(res):
    h = res.data.cpu().numpy()
    return [h[int(o):int(o) + int(n)].tobytes() for o, n in zip(res.offsets, res.lengths)]


def _kinds(findings):
    return [f.kind for f in findings]


def test_reference_pack(gpu_ctx):
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.pack import parse_header
    from rustic_core_amd.read import check_pack, read_blobs
    key, pack, blobs, _ = reference_pack(oracle)
    hlen = int.from_bytes(pack[-4:], "little")
    k = Key(key)
    entries = parse_header(k.decrypt_data(pack[-4 - hlen:-4]))
    assert len(entries) == len(blobs)  # (the fixture's blobs are stored, not compressed)
    want = [zr.decompress(p) if ulen else p for _, p, _, _, ulen in blobs]
    assert [hashlib.sha256(w).digest() for w in want] == [b[2] for b in blobs]
    assert _plain(read_blobs(k, _dev(pack), entries)) == want
    assert check_pack(k, _index_pack(pack, entries), pack) == []
    assert check_pack(k, _index_pack(pack, entries), _dev(pack)) == []


SIZES = [1, 17, 4096, 70000, 131073, 300001, 5000, 262144]


def _device_pack(gpu_ctx, key, seed=21, ulen_add=None, wrong_id=None, bad_frame=None):
    """One pack of SIZES blobs, every second one compressed on the device;
    returns (pack bytes, header entries, original blobs).  ulen_add / wrong_id
    / bad_frame tamper with what the packer is given for one blob."""
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.pack import parse_header
    rng = np.random.default_rng(seed)
    origs = [_data(rng, n, k) for n, k in zip(SIZES, ["text", "random", "csv", "mixed", "text",
                                                      "text", "binary", "periodic"])]
    comp = [i % 2 == 1 or i == 0 for i in range(len(origs))]
    frames = _device_frames(gpu_ctx, [o for o, c in zip(origs, comp) if c])
    it = iter(frames)
    datas = [next(it) if c else o for o, c in zip(origs, comp)]
    assert len(zr.blocks(datas[SIZES.index(300001)])) >= 3
    if bad_frame is not None:
        f = bytearray(datas[bad_frame])
        f[0] ^= 1  # the magic
        datas[bad_frame] = bytes(f)
    specs = []
    for i, (o, c) in enumerate(zip(origs, comp)):
        bid = hashlib.sha256(o).digest()
        if wrong_id == i:
            bid = bytes([bid[0] ^ 1]) + bid[1:]
        ulen = (len(o) + (ulen_add[1] if ulen_add and ulen_add[0] == i else 0)) if c else 0
        specs.append((0, np.frombuffer(bid, np.uint8),
                      bytes(rng.integers(0, 256, 16, dtype=np.uint8)), ulen))
    hn = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    files, _, _, _, _ = _build(key, datas, specs, [(0, len(datas))], [hn])
    pack = files[0]
    hlen = int.from_bytes(pack[-4:], "little")
    entries = parse_header(Key(key).decrypt_data(pack[-4 - hlen:-4]))
    return pack, entries, origs


KEY = bytes(range(64))


def test_device_built_pack(gpu_ctx):
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.read import check_pack, read_blobs
    pack, entries, origs = _device_pack(gpu_ctx, KEY)
    k = Key(KEY)
    assert sum(1 for e in entries if e.uncompressed_len) == 5
    assert check_pack(k, _index_pack(pack, entries), pack) == []
    assert _plain(read_blobs(k, _dev(pack), entries)) == origs
    # index.IndexBlob-shaped entries, a subset, another order
    ip = _index_pack(pack, entries)
    pick = [ip.blobs[i] for i in (5, 0, 3)]
    assert _plain(read_blobs(k, _dev(pack), pick)) == [origs[i] for i in (5, 0, 3)]
    assert _plain(read_blobs(k, _dev(pack), [])) == []


def test_check_pack_findings(gpu_ctx):
    """One tampering per CheckError, in check.rs's order."""
    import copy
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.read import check_pack
    k = Key(KEY)
    pack, entries, _ = _device_pack(gpu_ctx, KEY)
    ip = _index_pack(pack, entries)
    # a pack cut by a byte
    assert _kinds(check_pack(k, ip, pack[:-1])) == ["PackSizeMismatch"]
    # a flipped byte
    flipped = bytearray(pack)
    flipped[1000] ^= 4
    assert _kinds(check_pack(k, ip, bytes(flipped))) == ["PackHashMismatch"]
    # a wrong trailing length (the id recomputed: the hash step passes)
    hl = int.from_bytes(pack[-4:], "little")
    wrong = pack[:-4] + (hl + 4).to_bytes(4, "little")
    f = check_pack(k, _index_pack(wrong, entries), wrong)
    assert _kinds(f) == ["PackHeaderLengthMismatch"]
    assert (f[0].fields["length"], f[0].fields["computed"]) == (hl + 4, hl)
    # an index entry with another offset
    ip2 = copy.deepcopy(ip)
    ip2.blobs[2].offset += 1
    assert _kinds(check_pack(k, ip2, pack)) == ["PackHeaderMismatchIndex"]
    # an uncompressed_length off by one (header and index agree on it)
    target = 3  # a compressed blob
    for add in (1, -1):
        p, e, _ = _device_pack(gpu_ctx, KEY, ulen_add=(target, add))
        f = check_pack(k, _index_pack(p, e), p)
        assert _kinds(f) == ["PackBlobLengthMismatch"]
        assert f[0].fields["blob_id"] == e[target].id
    # a blob id changed (header and index agree on it)
    for target in (3, 4):  # compressed, stored
        p, e, origs = _device_pack(gpu_ctx, KEY, wrong_id=target)
        f = check_pack(k, _index_pack(p, e), p)
        assert _kinds(f) == ["PackBlobHashMismatch"]
        assert f[0].fields["comp_id"] == hashlib.sha256(origs[target]).digest()


def test_errors_that_raise(gpu_ctx):
    from rustic_core_amd.compress import DECODE_MESSAGE
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.pack import HeaderBlob
    from rustic_core_amd.read import check_pack, read_blobs
    k = Key(KEY)
    pack, entries, _ = _device_pack(gpu_ctx, KEY)
    # a flipped ciphertext byte of a blob, the pack id recomputed: the MAC
    bad = bytearray(pack)
    bad[entries[3].offset + 20] ^= 1
    bad = bytes(bad)
    for call in (lambda: check_pack(k, _index_pack(bad, entries), bad),
                 lambda: read_blobs(k, _dev(bad), entries)):
        with pytest.raises(RusticError) as e:
            call()
        assert e.value.kind == ErrorKind.Cryptography and "MAC check failed" in e.value.message
    with pytest.raises(RusticError):
        k.decrypt_data(bad[entries[3].offset:entries[3].offset + entries[3].length])
    # a corrupted frame under a valid MAC
    p, e, _ = _device_pack(gpu_ctx, KEY, bad_frame=5)
    for call in (lambda: check_pack(k, _index_pack(p, e), p), lambda: read_blobs(k, _dev(p), e)):
        with pytest.raises(RusticError) as err:
            call()
        assert err.value.kind == ErrorKind.Internal and err.value.message == DECODE_MESSAGE
    # read_encrypted_from_partial's length check, both ways
    for add in (1, -1):
        e2 = [HeaderBlob(b.type, b.offset, b.length, b.uncompressed_len + (add if i == 3 else 0), b.id)
              for i, b in enumerate(entries)]
        with pytest.raises(RusticError) as err:
            read_blobs(k, _dev(pack), e2)
        assert err.value.kind == ErrorKind.Internal
        assert "does not match the given length" in err.value.message
