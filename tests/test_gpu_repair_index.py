"""headers.repair_index and headers.index_checked on the device, over a
repository the device packer built: data and tree packs, some entries
compressed.  The index files written are read back with IndexFile.from_json
and held against the packs' contents and against ``repair_index(device=None)``."""
import hashlib
import warnings

import numpy as np
import pytest

from oracle import zstd_ref as zr
from tests.test_gpu_pack import _build

pytestmark = pytest.mark.gpu

KEY = bytes(range(64))
# blobs per pack and their type: one type per pack
GROUPS = [(0, 8), (0, 5), (1, 6), (1, 3), (0, 1), (1, 40)]


class Built:
    def __init__(self):
        from rustic_core_amd.crypto import Key
        from rustic_core_amd.index import IndexPack
        from rustic_core_amd.pack import parse_header
        rng = np.random.default_rng(17)
        datas, specs, groups = [], [], []
        for tpe, n in GROUPS:
            groups.append((len(datas), n))
            for k in range(n):
                d = rng.integers(0, 256, int(rng.integers(1, 400)), dtype=np.uint8).tobytes()
                datas.append(d)
                # every third blob counts as compressed: its raw length goes to the header
                specs.append((tpe, np.frombuffer(hashlib.sha256(d).digest(), np.uint8),
                              bytes(rng.integers(0, 256, 16, dtype=np.uint8)),
                              3 * len(d) + 1 if k % 3 == 0 else 0))
        files, _, _, _, _ = _build(KEY, datas, specs, groups,
                                   [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in groups])
        self.key = Key(KEY)
        self.packs, self.index_packs = {}, []
        for pack in files:
            hlen = int.from_bytes(pack[-4:], "little")
            ip = IndexPack(hashlib.sha256(pack).digest())
            for e in parse_header(self.key.decrypt_data(pack[-4 - hlen:-4])):
                ip.add(e.id, e.type, e.offset, e.length, e.uncompressed_len or None)
            self.packs[ip.id] = pack
            self.index_packs.append(ip)
        assert [(p.blobs[0].type, len(p.blobs)) for p in self.index_packs] == GROUPS
        assert any(b.uncompressed_length for p in self.index_packs for b in p.blobs)

    def listed(self, packs=None):
        return {i: len(p) for i, p in (packs or self.packs).items()}

    def reader(self, packs=None):
        from rustic_core_amd.restore import from_packs
        return from_packs(packs or self.packs)


_BUILT = {}


@pytest.fixture
def built(gpu_ctx):
    if "b" not in _BUILT:  # one repository for the whole module, never changed
        _BUILT["b"] = Built()
    return _BUILT["b"]


class Backend:
    """What repair_index writes and removes."""

    def __init__(self):
        self.files, self.removed = {}, []

    def save(self, ids, sealed, offs, lens):
        host = sealed.cpu().numpy()
        for i, o, n in zip(ids, offs, lens):
            data = host[int(o):int(o) + int(n)].tobytes()
            assert hashlib.sha256(data).digest() == bytes(i)
            self.files[bytes(i)] = data

    def texts(self, key):
        out = []
        for data in self.files.values():
            plain = key.decrypt_data(data)
            assert plain[:1] == b"\x02"
            out.append(zr.decompress(plain[1:], 1 << 22))
        return out


def _host_repair(built, files, packs=None, **kw):
    from rustic_core_amd.headers import repair_index
    saved, removed = [], []

    def save(f):
        saved.append(f.to_json())
        return hashlib.sha256(saved[-1]).digest()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rep = repair_index(built.key, files, built.listed(packs), built.reader(packs), save,
                           removed.append, device=None, **kw)
    return rep, saved, removed


def test_read_all_rebuilds_the_index(built):
    from rustic_core_amd.headers import repair_index
    from rustic_core_amd.index import IndexFile, IndexPack
    timed = [IndexPack(p.id, p.blobs, time="2024-05-06T07:08:09+02:00") for p in built.index_packs]
    files = [(hashlib.sha256(b"index:0").digest(), IndexFile(timed[:4])),
             (hashlib.sha256(b"index:1").digest(), IndexFile(timed[4:]))]
    be = Backend()
    rep = repair_index(built.key, files, built.listed(), built.reader(), be.save, be.removed.append,
                       read_all=True)
    assert rep.modified == [i for i, _ in files] == be.removed
    assert rep.read == [p.id for p in built.index_packs] and rep.failed == [] and rep.dropped == []
    assert rep.saved == list(be.files) and len(be.files) == 1
    texts = be.texts(built.key)
    # exactly the packs' contents: no time, no size, no delete mark
    got = IndexFile.from_json(texts[0])
    assert got.packs == built.index_packs and not got.packs_to_delete and got.supersedes is None
    # one type per pack: byte-equal to the host rule
    rep_h, saved_h, removed_h = _host_repair(built, files, read_all=True)
    assert texts == saved_h and removed_h == be.removed
    assert (rep_h.modified, rep_h.read, rep_h.dropped) == (rep.modified, rep.read, rep.dropped)


def _damaged(built):
    """(index files, packs): pack 1 in no index file, pack 2's size in the
    index falsified, pack 3's header corrupted and its index size falsified
    too (so that it is read)."""
    from rustic_core_amd.index import IndexFile, IndexPack
    ips = built.index_packs
    packs = dict(built.packs)
    bad = bytearray(packs[ips[3].id])
    bad[-4 - 20] ^= 0x40  # a byte of the sealed header
    packs[ips[3].id] = bytes(bad)
    files = [(hashlib.sha256(b"index:a").digest(),
              IndexFile([ips[0], IndexPack(ips[2].id, ips[2].blobs, size=len(packs[ips[2].id]) + 1)])),
             (hashlib.sha256(b"index:b").digest(),
              IndexFile([IndexPack(ips[3].id, ips[3].blobs, size=7), ips[4]], [ips[5]]))]
    return files, packs


def test_repair_of_a_damaged_index(built):
    from rustic_core_amd.errors import ErrorKind
    from rustic_core_amd.headers import repair_index
    from rustic_core_amd.index import IndexFile
    ips = built.index_packs
    files, packs = _damaged(built)
    be = Backend()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rep = repair_index(built.key, files, built.listed(packs), built.reader(packs), be.save,
                           be.removed.append)
    assert rep.modified == [i for i, _ in files] == be.removed and rep.dropped == []
    assert rep.read == [ips[2].id, ips[1].id]            # re-read, then the one listed only
    assert [i for i, _ in rep.failed] == [ips[3].id]      # reported and left out
    assert rep.failed[0][1].kind == ErrorKind.Cryptography
    assert any(ips[3].id.hex() in str(x.message) for x in w)
    assert rep.saved == list(be.files) and len(be.files) == 3
    got = [IndexFile.from_json(t) for t in be.texts(built.key)]
    assert [f.packs for f in got] == [[ips[0]], [ips[4]], [ips[2], ips[1]]]
    assert [f.packs_to_delete for f in got] == [[], [ips[5]], []]
    # the host rule writes the same three files
    rep_h, saved_h, _ = _host_repair(built, files, packs)
    assert be.texts(built.key) == saved_h
    assert (rep_h.read, [i for i, _ in rep_h.failed]) == (rep.read, [ips[3].id])


def test_dry_run_writes_and_removes_nothing(built):
    from rustic_core_amd.headers import repair_index
    files, packs = _damaged(built)
    be = Backend()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rep = repair_index(built.key, files, built.listed(packs), built.reader(packs), be.save,
                           be.removed.append, dry_run=True)
    assert be.files == {} and be.removed == [] and rep.saved == []
    assert rep.modified == [i for i, _ in files]
    assert rep.read == [built.index_packs[2].id, built.index_packs[1].id]
    assert [i for i, _ in rep.failed] == [built.index_packs[3].id]


def _lookups(dx, packs):
    """Per blob: (type, pack id, offset, length, uncompressed length, count)."""
    out = []
    for t in (0, 1):
        blobs = [b for p in packs for b in p.blobs if b.type == t]
        ids = np.frombuffer(b"".join(b.id for b in blobs), np.uint8).reshape(-1, 32)
        hits = dx.lookup(t, ids).cpu().numpy().view(np.uint32)
        names = dx.packs(t)
        for b, h in zip(blobs, hits):
            assert int(h[0]) != 0xFFFFFFFF, b.id.hex()
            out.append((t, names[int(h[2])], int(h[3]), int(h[4]), int(h[5]), int(h[1])))
    return out


def test_index_checked(built):
    from rustic_core_amd import DeviceIndex
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.headers import index_checked
    from rustic_core_amd.index import IndexFile
    ips = built.index_packs
    files, packs = _damaged(built)
    with pytest.raises(RusticError) as e:
        index_checked(built.key, [f for _, f in files], built.listed(packs), built.reader(packs))
    assert e.value.kind == ErrorKind.Cryptography
    # the same index files over the packs as they were: pack 3 is read too, and reads well
    dx = index_checked(built.key, [f for _, f in files], built.listed(), built.reader())
    # a pack in packs_to_delete that the listing confirms is neither collected nor read
    true = DeviceIndex.from_index_files([IndexFile(ips[:5], [ips[5]])])
    assert _lookups(dx, ips[:5]) == _lookups(true, ips[:5])
    for t in (0, 1):
        assert sorted(dx.packs(t)) == sorted(true.packs(t))
        assert dx.total_size(t) == true.total_size(t) and dx.size(t) == true.size(t)
        assert not dx.has(t, ips[5].blobs[0].id)
    # the kept packs first, then the headers in the order read
    assert dx.packs(0) == [ips[0].id, ips[4].id, ips[1].id]
    assert dx.packs(1) == [ips[2].id, ips[3].id]
    dx.close()
    true.close()
