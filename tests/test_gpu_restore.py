"""Restore of file contents on the device (rustic_core_amd/restore.py): what
the native ingest engine backed up comes back byte for byte through
RestorePlan.add_file (commands/restore.rs:744-837), pack_reads (:561-583) and
restore_contents (:530-677) -- whole files, sparse, over existing files,
from other files that hold the blob already, in batches, and with the errors
of read_blobs."""
import copy

import numpy as np
import pytest

from tests.test_gpu_native_ingest import KEY, _files, _run
from tests.test_gpu_read import _dev

pytestmark = pytest.mark.gpu

MIN, AVG, MAX = 4096, 16384, 65536


def _inputs():
    rng = np.random.default_rng(77)
    f0 = rng.integers(0, 256, 300001, dtype=np.uint8)
    h1, h2 = rng.integers(0, 256, 90000, dtype=np.uint8), rng.integers(0, 256, 70001, dtype=np.uint8)
    return [f0, _files()[7][:400000].copy(),
            np.concatenate([h1, np.zeros(200000, np.uint8), h2]),
            f0.copy(), np.zeros(0, np.uint8), rng.integers(0, 256, 100, dtype=np.uint8)]


class Backup:
    def __init__(self, level):
        from oracle import oracle
        from rustic_core_amd.chunker import Context
        from rustic_core_amd.index import IndexFile, IndexPack
        from rustic_core_amd.restore import index_lookup
        ctx = Context.get(oracle.DEFAULT_POLY, MIN, AVG, MAX, device=0)
        self.files = _inputs()
        # 128 KiB packs: what is unique here (two random files; the text and
        # the zeros dedup to a few blobs) is about 460 KB, which is only two
        # packs of 256 KiB, and the tests want at least three
        ing, _ = _run(ctx, self.files, level=level, pack_size=128 << 10, pack_grow_factor=0)
        try:
            self.packs = {p["id"]: p["data"] for p in ing.packs}
            self.index_files = []
            for p in ing.packs:
                ip = IndexPack(p["id"])
                for bid, off, ln, ulen, tpe in p["blobs"]:
                    ip.add(bid, tpe, off, ln, ulen or None)
                self.index_files.append(IndexFile([ip]))
            self.contents = []   # per file: [(blob id, start, length)]
            for i in range(len(self.files)):
                cuts, ids, _, ln = ing.files[i]
                assert ln == self.files[i].size
                starts = np.concatenate([[0], cuts[:-1]]).astype(np.int64) if len(cuts) else []
                self.contents.append([(bytes(ids[j]), int(starts[j]), int(cuts[j]) - int(starts[j]))
                                      for j in range(len(cuts))])
        finally:
            ing.close()
        self.index = index_lookup(self.index_files)
        self.level = level

    def ids(self, i):
        return [c[0] for c in self.contents[i]]

    def plan(self, which=None, existing=None):
        from rustic_core_amd.restore import RestorePlan
        plan, results = RestorePlan(), []
        for i in (range(len(self.files)) if which is None else which):
            results.append(plan.add_file(f"f{i}", self.files[i].size, self.ids(i), self.index,
                                         existing=(existing or {}).get(i)))
        return plan, results

    def reader(self, packs=None):
        from rustic_core_amd.restore import from_packs
        inner, calls = from_packs(packs or self.packs), []

        def read_partial(pack_id, offset, length):
            calls.append((pack_id, offset, length))
            return inner(pack_id, offset, length)
        return read_partial, calls


_BACKUPS = {}


def _backup(level):
    if level not in _BACKUPS:   # one backup per level for the whole module, never changed
        _BACKUPS[level] = Backup(level)
    return _BACKUPS[level]


@pytest.fixture(params=[0, None], ids=["zstd", "stored"])
def backup(request, gpu_ctx):
    return _backup(request.param)


@pytest.fixture
def backup0(gpu_ctx):
    return _backup(0)


def _key():
    from rustic_core_amd.crypto import Key
    return Key(KEY)


def _same(t, data):
    return np.array_equal(t.cpu().numpy(), data)


def test_round_trip(backup):
    """Both repository versions: zstd blobs with an uncompressed length, and
    stored blobs without one."""
    from rustic_core_amd.restore import restore_contents
    b = backup
    assert len(b.packs) >= 3
    plan, results = b.plan()
    assert results == ["Modify"] * len(b.files)
    assert any(len(fls) >= 2 for fls in plan.r.values())   # dedup: one blob, two positions
    assert plan.file_lengths == [f.size for f in b.files]
    assert plan.restore_size == sum(n for c in b.contents for _, _, n in c)
    assert plan.matched_size == 0
    ul = [k[3] for k in plan.r]
    assert all(ul) if b.level is not None else not any(ul)
    read_partial, calls = b.reader()
    res = restore_contents(_key(), plan, read_partial)
    for t, f in zip(res.files, b.files):
        assert _same(t, f)
    reads = plan.pack_reads()
    assert all(r.from_file is None for r in reads)
    assert calls == [(r.pack_id, r.offset, r.length) for r in reads]
    assert len(calls) < len(plan.r)   # neighbours were coalesced
    assert plan.to_packs() == sorted(b.packs)
    assert res.holes == []


def _zero_chunks(b):
    return sorted((i, s, n) for i, c in enumerate(b.contents) for _, s, n in c
                  if not b.files[i][s:s + n].any())


def test_sparse(backup0):
    from rustic_core_amd.restore import restore_contents
    b = backup0
    want = _zero_chunks(b)
    assert len(want) >= 1
    plan, _ = b.plan()
    dense = restore_contents(_key(), plan, b.reader()[0])
    sparse = restore_contents(_key(), plan, b.reader()[0], sparse=True)
    for t, f in zip(sparse.files, b.files):
        assert _same(t, f)   # new tensors start from zeros
    assert sparse.holes == want and dense.holes == []
    # zero_blobs counts blobs, not positions: every all-zero chunk of the same
    # length is one blob
    n_zero = len({c[0] for i, s, n in want for c in b.contents[i] if c[1] == s})
    assert sparse.zero_blobs == dense.zero_blobs == n_zero


def test_existing_identical_and_one_byte_flipped(backup0):
    from rustic_core_amd.restore import restore_contents
    b = backup0
    # identical: nothing of the file is read
    e0 = _dev(b.files[0].tobytes())
    plan, results = b.plan([0, 5], existing={0: e0})
    assert results == ["Verified", "Modify"]
    assert plan.matched_size == b.files[0].size and plan.restore_size == 100
    read_partial, calls = b.reader()
    res = restore_contents(_key(), plan, read_partial)
    assert res.files[0].data_ptr() == e0.data_ptr()
    assert _same(res.files[0], b.files[0]) and _same(res.files[1], b.files[5])
    f0_blobs = {(b.index[i][0], b.index[i][1].offset) for i in b.ids(0)}
    for r in plan.pack_reads():
        if (r.pack_id, r.offset, r.length) in calls:
            assert not any((r.pack_id, bl.offset) in f0_blobs for bl, dests in r.blobs if dests)
    assert len(calls) == 1
    # one byte flipped in the second chunk: exactly that chunk is restored
    bid, s, n = b.contents[0][1]
    bad = b.files[0].copy()
    bad[s + n // 2] ^= 0x40
    e1 = _dev(bad.tobytes())
    plan, results = b.plan([0], existing={0: e1})
    assert results == ["Modify"]
    assert plan.restore_size == n and plan.matched_size == b.files[0].size - n
    read_partial, calls = b.reader()
    res = restore_contents(_key(), plan, read_partial)
    pack, ib = b.index[bid]
    # one read, from that blob on (matching neighbours coalesce into it, as in
    # the reference, but only the blob with a destination is opened)
    reads = [r for r in plan.pack_reads() if any(d for _, d in r.blobs)]
    assert [(bl.offset, d) for r in reads for bl, d in r.blobs if d] == [(ib.offset, [(0, s)])]
    assert calls == [(r.pack_id, r.offset, r.length) for r in reads]
    assert len(calls) == 1 and calls[0][:2] == (pack, ib.offset)
    assert res.files[0].data_ptr() == e1.data_ptr() and _same(e1, b.files[0])


def test_duplicate_file_filled_from_the_present_one(backup0):
    """File 3 is a copy of file 0, which is at the destination and intact:
    every blob of file 3 comes out of files[0] (from_file), none from a pack."""
    from rustic_core_amd.restore import restore_contents
    b = backup0
    e0 = _dev(b.files[0].tobytes())
    plan, results = b.plan([0, 3], existing={0: e0})
    assert results == ["Verified", "Modify"]
    reads = plan.pack_reads()
    assert reads and all(r.from_file is not None and r.from_file[0] == 0 for r in reads)
    assert plan.to_packs() == []
    read_partial, calls = b.reader()
    res = restore_contents(_key(), plan, read_partial)
    assert calls == []
    assert res.files[0].data_ptr() == e0.data_ptr()
    assert _same(res.files[0], b.files[0]) and _same(res.files[1], b.files[3])


def test_existing_of_another_size_and_empty(backup0):
    from rustic_core_amd.restore import RestorePlan, restore_contents
    b = backup0
    short = _dev(b.files[5].tobytes()[:-1])
    plan, results = b.plan([5], existing={5: short})
    assert results == ["Modify"] and plan.restore_size == 100 and plan.matched_size == 0
    res = restore_contents(_key(), plan, b.reader()[0])
    assert res.files[0].data_ptr() != short.data_ptr() and _same(res.files[0], b.files[5])
    plan = RestorePlan()
    assert plan.add_file("empty", 0, [], b.index, existing=b"") == "Existing"
    assert plan.names == [] and plan.file_lengths == []
    assert plan.add_file("empty", 0, [], b.index) == "Modify"   # absent: it is created
    assert plan.file_lengths == [0]
    # bytes are uploaded
    assert plan.add_file("f5", 100, b.ids(5), b.index, existing=b.files[5].tobytes()) == "Verified"


def test_batches(backup0):
    from rustic_core_amd.restore import _groups, restore_contents
    b = backup0
    plan, _ = b.plan()
    groups = _groups(plan.pack_reads(), 100_000)
    sizes = [sum(bl.uncompressed_length for r in g for bl, d in r.blobs if d) for g in groups]
    assert len(groups) >= 3 and any(len(g) == 1 and n > 100_000 for g, n in zip(groups, sizes))
    assert all(n <= 100_000 or len(g) == 1 for g, n in zip(groups, sizes))
    read_partial, calls = b.reader()
    res = restore_contents(_key(), plan, read_partial, batch_bytes=100_000)
    for t, f in zip(res.files, b.files):
        assert _same(t, f)
    assert calls == [(r.pack_id, r.offset, r.length) for r in plan.pack_reads()]
    # device tensors as read_partial results
    dev_packs = {k: _dev(v) for k, v in b.packs.items()}
    res = restore_contents(_key(), plan, b.reader(dev_packs)[0], batch_bytes=100_000, sparse=True)
    for t, f in zip(res.files, b.files):
        assert _same(t, f)


def test_errors(backup0):
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.restore import index_lookup, restore_contents
    b = backup0
    plan, _ = b.plan()
    bid = b.ids(1)[2]
    pack, ib = b.index[bid]
    bad = bytearray(b.packs[pack])
    bad[ib.offset + 20] ^= 1
    with pytest.raises(RusticError) as e:
        restore_contents(_key(), plan, b.reader({**b.packs, pack: bytes(bad)})[0])
    assert e.value.kind == ErrorKind.Cryptography and "MAC check failed" in e.value.message
    # an index entry whose uncompressed_length is off by one
    files = copy.deepcopy(b.index_files)
    for f in files:
        for blob in f.packs[0].blobs:
            if blob.id == bid:
                blob.uncompressed_length += 1
    from rustic_core_amd.restore import RestorePlan
    plan = RestorePlan()
    plan.add_file("f1", b.files[1].size, b.ids(1), index_lookup(files))
    with pytest.raises(RusticError) as e:
        restore_contents(_key(), plan, b.reader()[0])
    assert e.value.kind == ErrorKind.Internal
    assert "does not match the given length" in e.value.message
