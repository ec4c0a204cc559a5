"""GPU: rustic_core_amd.check on the device -- the reference's eight recorded
repositories through check_repository(device=0), and check_pack_batch over
device-built packs against the loop over read.check_pack."""
import copy
import hashlib

import numpy as np
import pytest

from oracle import oracle, zstd_ref as zr
from tests.check_cases import INACTIVE, REPOS, normal, recorded, run
from tests.test_gpu_pack import _build

pytestmark = pytest.mark.gpu
KEY = bytes(range(64))
SIZES = [1, 17, 4096, 7000, 1300, 20001, 500, 2600]


@pytest.mark.parametrize("name", REPOS)
def test_fixture_results_on_the_device(gpu_ctx, name):
    """The same expectations as tests/test_check_host.py, through
    rcdc_check_packs, DeviceIndex lookups, the batched tree reads and
    check_pack_batch."""
    from rustic_core_amd.crypto import Key
    got = normal(run(name, oracle, Key, 0, snapshot_trees_device=0))
    assert got == recorded(name)
    if name == INACTIVE:
        assert got[-1][2]["file"] == "home/thinkpad/data/test"


def test_check_packs_device_equals_host(gpu_ctx):
    """check_packs and check_packs_entries over packs with gaps, shuffled
    blobs, wrong types and one pack the kernel leaves to the host."""
    import torch
    from rustic_core_amd.check import PackRecord, _flatten, check_packs, check_packs_entries, sort_max
    from rustic_core_amd.index import IndexFile, IndexPack
    from tests import ckpack_model as cm
    rng = np.random.default_rng(8)
    f = IndexFile()
    for i, n in enumerate([40, 0, 300, sort_max() + 5, 7]):
        ids, locs, tps = cm.random_pack(rng, n, shuffle=i != 0, gap=i % 2 == 0, types=i & 1)
        if n > 10:
            tps[n // 2] ^= 1
        p = IndexPack(bytes([i + 1]) * 32, time=None if i == 4 else "2024-01-01T00:00:00Z")
        for a, l, t in zip(ids, locs, tps):
            p.add(bytes(a), int(t), int(l[1]), int(l[2]), int(l[3]) or None)
        f.add(p, delete=i >= 3)
    listed = [(bytes([1]) * 32, 5), (bytes([9]) * 32, 5)]
    want = check_packs([f], listed, listed, device=None)
    got = check_packs([f], listed, listed, device=0)
    assert got == want and len(want[0]) > 150
    assert "PackTimeNotSet" in [x.kind for _, x in want[0]]
    packs = f.packs + f.packs_to_delete
    ids, locs, tps, ranges = _flatten(packs)
    d = lambda a: torch.from_numpy(a).to("cuda:0")
    d_locs = d(locs.view(np.int32))
    recs = [PackRecord(p.id, fr, c, k >= 3, p.time is not None) for k, (p, (fr, c)) in
            enumerate(zip(packs, ranges))]
    found, missing = check_packs_entries((d(ids), d_locs[:, 1], d_locs[:, 2], d_locs[:, 3], d(tps)),
                                         recs, listed, listed)
    assert found == want[0] and missing == want[2]


def _pack(seed, ulen_add=None, wrong_id=None, bad_frame=None, types=None, sizes=SIZES):
    """One device-built pack of ``sizes`` blobs, every second one a zstd
    frame; returns (pack bytes, its IndexPack)."""
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.index import IndexPack
    from rustic_core_amd.pack import parse_header
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, 6, dtype=np.uint8)) for _ in range(50)]
    origs = [b" ".join(words[int(x)] for x in rng.integers(0, 50, n // 7 + 1))[:n] for n in sizes]
    comp = [i % 2 == 1 for i in range(len(origs))]
    datas = [zr.compress(o) if c else o for o, c in zip(origs, comp)]
    if bad_frame is not None:
        fr = bytearray(datas[bad_frame])
        fr[0] ^= 1  # the magic
        datas[bad_frame] = bytes(fr)
    specs = []
    for i, (o, c) in enumerate(zip(origs, comp)):
        bid = hashlib.sha256(o).digest()
        if wrong_id == i:
            bid = bytes([bid[0] ^ 1]) + bid[1:]
        ulen = (len(o) + (ulen_add[1] if ulen_add and ulen_add[0] == i else 0)) if c else 0
        specs.append((types[i] if types else 0, np.frombuffer(bid, np.uint8),
                      bytes(rng.integers(0, 256, 16, dtype=np.uint8)), ulen))
    hn = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    files, _, _, _, _ = _build(KEY, datas, specs, [(0, len(datas))], [hn])
    return files[0], _index(files[0])


def _index(pack: bytes, pid=None):
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.index import IndexPack
    from rustic_core_amd.pack import parse_header
    hlen = int.from_bytes(pack[-4:], "little")
    ip = IndexPack(hashlib.sha256(pack).digest() if pid is None else pid)
    for e in parse_header(Key(KEY).decrypt_data(pack[-4 - hlen:-4])):
        ip.add(e.id, e.type, e.offset, e.length, e.uncompressed_len or None)
    return ip


class CountingKey:
    """A key that counts its open_blobs calls."""

    def __init__(self, key):
        self.key, self.opens = key, 0

    def open_blobs(self, *a, **kw):
        self.opens += 1
        return self.key.open_blobs(*a, **kw)

    def __getattr__(self, name):
        return getattr(self.key, name)


def _norm(results):
    out = []
    for level, f in results:
        fields = dict(f.fields)
        if "source" in fields:
            e = fields["source"]
            fields["source"] = (getattr(e, "kind", None), getattr(e, "message", str(e)))
        out.append((level, f.kind, fields))
    return out


def _cases():
    """(name, IndexPack, bytes read or an exception) per pack: a clean pack
    and one for every finding kind and every raising case."""
    from rustic_core_amd.crypto import Key
    k = Key(KEY)
    pack, ip = _pack(21)
    cases = [("clean", ip, pack)]
    cut, i_cut = _pack(40)
    cases.append(("size", i_cut, cut[:-1]))
    flipped, i_flipped = _pack(41)
    flipped = bytearray(flipped)
    flipped[1000] ^= 4
    cases.append(("hash", i_flipped, bytes(flipped)))
    hl = int.from_bytes(pack[-4:], "little")
    wrong = pack[:-4] + (hl + 4).to_bytes(4, "little")
    cases.append(("header length", _index(pack, hashlib.sha256(wrong).digest()), wrong))
    p2, i2 = _pack(22)
    moved = copy.deepcopy(i2)
    moved.blobs[2].offset += 1
    cases.append(("header mismatch", moved, p2))
    for seed, add in ((23, 1), (24, -1)):
        cases.append((f"blob length {add}",) + _pack(seed, ulen_add=(3, add))[::-1])
    for seed, target in ((25, 3), (26, 4)):
        cases.append((f"blob hash {target}",) + _pack(seed, wrong_id=target)[::-1])
    cases.append(("clean 2",) + _pack(27)[::-1])
    # a blob's MAC (behind a blob with a finding of its own, which is kept), the header's MAC
    p3, i3 = _pack(28, wrong_id=0)
    bad = bytearray(p3)
    bad[i3.blobs[3].offset + 20] ^= 1
    cases.append(("blob mac", _index(p3, hashlib.sha256(bytes(bad)).digest()), bytes(bad)))
    p4, i4 = _pack(29)
    bad = bytearray(p4)
    bad[len(p4) - 4 - 10] ^= 1
    i4.id = hashlib.sha256(bytes(bad)).digest()
    cases.append(("header mac", i4, bytes(bad)))
    # a header whose first type byte is 4: the parser's status BAD_TYPE
    p5, i5 = _pack(30)
    hl = int.from_bytes(p5[-4:], "little")
    plain = bytearray(k.decrypt_data(p5[-4 - hl:-4]))
    plain[0] = 4
    p5 = p5[:-4 - hl] + k.encrypt_data(bytes(plain), bytes(16)) + p5[-4:]
    i5.id = hashlib.sha256(p5).digest()
    cases.append(("header status", i5, p5))
    cases.append(("bad frame",) + _pack(31, bad_frame=5)[::-1])
    cases.append(("mixed",) + _pack(32, types=[0, 1, 0, 0, 1, 0, 0, 0])[::-1])
    # an index that lists its blobs out of order: sorted on the device; then one too large for that
    p6, i6 = _pack(33)
    i6.blobs = i6.blobs[::-1]
    cases.append(("index out of order", i6, p6))
    from rustic_core_amd.check import sort_max
    p7, i7 = _pack(34, sizes=[1 + (i % 3) for i in range(sort_max() + 1)])
    i7.blobs = i7.blobs[1:] + i7.blobs[:1]
    cases.append(("host status", i7, p7))
    cases.append(("unreadable", _pack(35)[1], OSError("no such pack")))
    cases.append(("clean 3",) + _pack(36)[::-1])
    return cases


def test_check_pack_batch_equals_the_loop(gpu_ctx):
    """One batch with a clean pack and one pack for every finding kind and
    every raising case: the result is read.check_pack's per pack with its
    exceptions mapped, the clean packs beside a damaged one stay clean, the
    key sees at most two open_blobs calls per group beside the fallback
    packs', and splitting the batch into groups does not change the result."""
    from rustic_core_amd.check import ERROR, Finding, check_pack_batch
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.errors import RusticError
    from rustic_core_amd.read import check_pack
    cases = _cases()
    k = Key(KEY)
    data = {bytes(ip.id): d for _, ip, d in cases}
    assert len(data) == len(cases)

    def read_full(pid):
        if isinstance(data[pid], Exception):
            raise data[pid]
        return data[pid]
    want, per_case = [], {}
    for name, ip, d in cases:
        if isinstance(d, Exception):
            mine = [(ERROR, Finding("ErrorReadingPack", dict(id=bytes(ip.id), source=d)))]
        else:
            try:
                mine = [(ERROR, f) for f in check_pack(k, ip, d)]
            except RusticError as e:
                mine = [(ERROR, Finding("ErrorCheckingPack", dict(id=bytes(ip.id), source=e)))]
        per_case[name] = [kind for _, kind, _ in _norm(mine)]
        want += mine
    assert per_case == {
        "clean": [], "clean 2": [], "clean 3": [], "size": ["PackSizeMismatch"],
        "hash": ["PackHashMismatch"], "header length": ["PackHeaderLengthMismatch"],
        "header mismatch": ["PackHeaderMismatchIndex"],
        "blob length 1": ["PackBlobLengthMismatch"], "blob length -1": ["PackBlobLengthMismatch"],
        "blob hash 3": ["PackBlobHashMismatch"], "blob hash 4": ["PackBlobHashMismatch"],
        "blob mac": ["ErrorCheckingPack"], "header mac": ["ErrorCheckingPack"],
        "header status": ["ErrorCheckingPack"], "bad frame": ["ErrorCheckingPack"],
        "mixed": [], "index out of order": [], "host status": [],
        "unreadable": ["ErrorReadingPack"]}
    # read.check_pack raises at a pack's first failing blob and so gives none of that pack's
    # findings; the batch keeps those of the blobs before it: blob 0's wrong id here
    i_mac = [ip for name, ip, _ in cases if name == "blob mac"][0]
    kept = (ERROR, Finding("PackBlobHashMismatch",
                           dict(id=bytes(i_mac.id), blob_id=bytes(i_mac.blobs[0].id),
                                comp_id=bytes([i_mac.blobs[0].id[0] ^ 1]) + i_mac.blobs[0].id[1:])))
    at = [j for j, (_, f) in enumerate(want) if f.fields["id"] == bytes(i_mac.id)][0]
    want.insert(at, kept)
    packs = [ip for _, ip, _ in cases]
    ck = CountingKey(k)
    got = check_pack_batch(ck, packs, read_full)
    assert _norm(got) == _norm(want)
    fallback = 3  # header status, mixed, host status
    assert ck.opens <= 2 + 2 * fallback
    # several groups
    sizes = sorted(ip.pack_size() for ip in packs)
    for budget in (1, sizes[len(sizes) // 2] * 3):
        ck = CountingKey(k)
        again = check_pack_batch(ck, packs, read_full, budget=budget)
        assert _norm(again) == _norm(want), budget
    times = {}
    check_pack_batch(k, packs[:3], read_full, stage_times=times)
    assert set(times) >= {"pack_hash", "compare"}
