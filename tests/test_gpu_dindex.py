"""GPU: the blob index in device memory (rcdc_dindex, dindex.DeviceIndex)
against a Python dict and list built here, ingest.first_occurrences, and the
four tests of the reference's index/binarysorted.rs restated with packs of
our own.  The shapes are the smallest at which each mechanism can go wrong:
growth from an empty table, duplicates inside one launch, ids that share a
home slot, a probe that wraps, equal tags."""
import ctypes
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
NO_PACK = 0xFFFFFFFF


def sha(*parts) -> bytes:
    return hashlib.sha256(repr(parts).encode()).digest()


def arr(ids) -> np.ndarray:
    return np.frombuffer(b"".join(ids), np.uint8).reshape(len(ids), 32).copy()


class Raw:
    """rcdc_dindex through ctypes, with the dict and list it must agree with."""

    def __init__(self, ctx, reserve=0):
        import torch
        from rustic_core_amd import _lib
        self.torch, self.L, self._lib = torch, _lib.lib(), _lib
        self.h = ctypes.c_void_p()
        assert self.L.rcdc_dindex_create(ctx.handle, reserve, ctypes.byref(self.h)) == 0
        self.ids, self.locs = [], []      # the oracle: every entry in order
        self.first, self.count = {}, {}

    def close(self):
        self.L.rcdc_dindex_destroy(self.h)

    def _note(self, ids, locs):
        for k, i in enumerate(ids):
            self.first.setdefault(i, len(self.ids))
            self.count[i] = self.count.get(i, 0) + 1
            self.ids.append(i)
            self.locs.append(tuple(locs[k]) if locs is not None else (NO_PACK, 0, 0, 0))

    def add(self, ids, locs=None, device=False):
        a = arr(ids)
        l = None if locs is None else np.array(locs, np.uint32).reshape(len(ids), 4)
        if device:
            ta = self.torch.from_numpy(a).cuda()
            tl = None if l is None else self.torch.from_numpy(l.view(np.int32)).cuda()
            st = self.L.rcdc_dindex_add(self.h, ta.data_ptr(), None if tl is None else tl.data_ptr(),
                                        len(ids), 1, None)
        else:
            st = self.L.rcdc_dindex_add(self.h, a.ctypes.data, None if l is None else l.ctypes.data,
                                        len(ids), 0, None)
        assert st == 0, self._lib.last_error()
        self._note(ids, locs)

    def lookup(self, ids) -> np.ndarray:
        n = len(ids)
        q = self.torch.from_numpy(arr(ids)).cuda() if n else \
            self.torch.empty((0, 32), dtype=self.torch.uint8, device="cuda")
        hits = self.torch.full((max(n, 1), 6), 0x5A5A5A5A, dtype=self.torch.int32, device="cuda")
        st = self.L.rcdc_dindex_lookup(self.h, q.data_ptr() if n else None, n,
                                       hits.data_ptr() if n else None, None)
        assert st == 0, self._lib.last_error()
        self.torch.cuda.synchronize()
        return hits[:n].cpu().numpy().view(np.uint32).reshape(n, 6)

    def expect(self, ids) -> np.ndarray:
        out = np.zeros((len(ids), 6), np.uint32)
        for k, i in enumerate(ids):
            if i in self.first:
                e = self.first[i]
                out[k] = (e, self.count[i]) + self.locs[e]
            else:
                out[k] = (MISS, 0, 0, 0, 0, 0)
        return out

    def check(self, ids):
        got, want = self.lookup(ids), self.expect(ids)
        bad = np.nonzero((got != want).any(1))[0]
        assert not len(bad), (bad[:5], got[bad[:5]], want[bad[:5]])

    def size(self):
        return int(self.L.rcdc_dindex_size(self.h))

    def keys(self):
        return int(self.L.rcdc_dindex_keys(self.h))


@pytest.fixture
def raw(gpu_ctx):
    r = Raw(gpu_ctx)
    yield r
    r.close()


def _locs(n, base=0):
    return [((base + k) % 7, 3 * (base + k), 100 + (base + k) % 50, (base + k) % 3 * 11)
            for k in range(n)]


ABSENT = [sha("absent", k) for k in range(1000)]


def test_empty_and_one_entry(raw):
    raw.check(ABSENT[:300])                      # an empty index: all misses
    assert raw.lookup([]).shape == (0, 6)        # n = 0 queries
    assert raw.size() == 0 and raw.keys() == 0
    assert raw.L.rcdc_dindex_add(raw.h, None, None, 0, 0, None) == 0  # n = 0 adds nothing
    one = sha("one")
    raw.add([one], [(5, 6, 7, 8)])
    assert raw.size() == 1 and raw.keys() == 1
    raw.check([one] + ABSENT[:70] + [one])
    assert raw.lookup([one])[0].tolist() == [0, 1, 5, 6, 7, 8]


def test_growth_from_nothing(raw):
    """1, then 1 000, then 70 000 entries from reserve_entries = 0: the table
    and the entry arrays grow twice; everything added so far is found."""
    added = []
    for rnd, n in enumerate((1, 1000, 70000)):
        ids = [sha("grow", rnd, k) for k in range(n)]
        raw.add(ids, _locs(n, len(added)))
        added += ids
        assert raw.size() == len(added) == raw.keys()
        raw.check(added)
        raw.check(ABSENT)


def test_duplicates_in_one_launch(raw):
    ids8 = [sha("dup", k) for k in range(8)]
    ids = [ids8[k % 8] for k in range(4096)]
    raw.add(ids, _locs(4096))
    assert raw.size() == 4096 and raw.keys() == 8
    got = raw.lookup(ids8)
    assert got[:, 0].tolist() == list(range(8))          # the lowest entry of each id
    assert got[:, 1].tolist() == [512] * 8
    assert [tuple(r) for r in got[:, 2:]] == _locs(8)
    raw.check(ids8 + ABSENT[:50])
    more = [sha("dup-more", k) for k in range(70000)]
    raw.add(more, _locs(70000, 4096))                    # forces a growth: a rebuild
    assert raw.size() == 74096 and raw.keys() == 70008
    assert (raw.lookup(ids8) == got).all()
    raw.check(ids8 + more[::97] + ABSENT[:50])


def test_duplicates_across_calls_and_count_used():
    from rustic_core_amd import DeviceIndex
    from rustic_core_amd.dindex import DATA
    many, twice, absent = sha("many"), sha("twice"), sha("never")
    dx = DeviceIndex(0)
    for k in range(3):
        dx.add_ids(arr([many] * 100 + ([twice] if k else [])))
    assert dx.size(DATA) == 302 and dx.keys(DATA) == 2 and len(dx) == 302
    used = dx.count_used(DATA, arr([many, absent, twice, many]))
    assert str(used.dtype) == "torch.uint8"
    assert used.cpu().tolist() == [255, 0, 2, 255]
    h = dx.lookup(DATA, arr([many, twice, absent])).cpu().numpy().view(np.uint32)
    assert h[:, :3].tolist() == [[0, 300, NO_PACK], [200, 2, NO_PACK], [MISS, 0, 0]]
    assert dx.has(DATA, many) and not dx.has(DATA, absent)
    assert dx.get_id(DATA, many) is None     # id-only entries have no location
    dx.close()


def test_colliding_ids(raw):
    """Crafted ids: one home slot for 300 ids at any table size, a home at
    the last slot (the probe wraps), ids one byte apart, ids with equal
    tags.  All are found; their near misses are not."""
    same_home = [b"\x37\x13\x00\x00\x00\x00\x00\x00" + sha("home", k)[8:] for k in range(300)]
    last_slot = [b"\xff" * 8 + sha("last", k)[8:] for k in range(300)]
    base = sha("byte31")
    byte31 = [base, base[:31] + bytes([base[31] ^ 1])]
    t = sha("tag")
    same_tag = [t, t[:12] + sha("tag2")[12:]]
    ids = same_home + last_slot + byte31 + same_tag
    assert len(set(ids)) == len(ids)
    raw.add(ids, _locs(len(ids)))
    assert raw.keys() == len(ids)
    raw.check(ids)
    near = [same_home[0][:31] + b"\x00", last_slot[7][:20] + b"\x00" + last_slot[7][21:],
            base[:31] + bytes([base[31] ^ 2]), t[:12] + sha("tag3")[12:],
            b"\xff" * 32, b"\x37\x13" + b"\x00" * 30, b"\x00" * 32,
            same_home[5][:8] + same_home[6][8:12] + same_home[5][12:]]
    near = [i for i in near if i not in raw.first]
    assert len(near) >= 7
    assert (raw.lookup(near)[:, 0] == MISS).all()
    # the same ids again, and a growth on top: counts and first entries hold
    raw.add(ids[::-1])
    raw.check(ids + near)
    raw.add([sha("fill", k) for k in range(3000)])
    raw.check(ids + near)
    assert raw.lookup(ids)[:, 1].tolist() == [2] * len(ids)


def test_host_and_device_sources(gpu_ctx):
    ids = [sha("src", k % 900) for k in range(1500)]
    locs = _locs(1500)
    a, b = Raw(gpu_ctx), Raw(gpu_ctx)
    a.add(ids[:700], locs[:700])
    a.add(ids[700:], None)
    b.add(ids[:700], locs[:700], device=True)
    b.add(ids[700:], None, device=True)
    q = ids[::3] + ABSENT[:100]
    ga, gb = a.lookup(q), b.lookup(q)
    assert (ga == gb).all() and (ga == a.expect(q)).all()
    assert a.size() == b.size() == 1500 and a.keys() == b.keys() == 900
    a.close()
    b.close()


# ---- first_new --------------------------------------------------------------

def _first_new_case():
    rng = np.random.default_rng(11)
    values = [sha("fn", k) for k in range(100)]
    known = set(values[::2])
    ids = [values[int(k)] for k in rng.integers(0, 100, 1000)]
    return values, known, ids, rng


def test_first_new_matches_first_occurrences():
    from rustic_core_amd import DeviceIndex
    from rustic_core_amd.dindex import DATA
    from rustic_core_amd.ingest import first_occurrences
    values, known, ids, rng = _first_new_case()
    a = arr(ids)
    dx = DeviceIndex(0)
    dx.add_ids(arr(sorted(known)))
    before = dx.lookup(DATA, arr(values)).cpu().numpy()
    selects = [None, rng.integers(0, 2, 1000).astype(np.uint8)]
    # a select that leaves out the first occurrence of the unknown ids
    skip = np.ones(1000, np.uint8)
    left_out = [v for v in values[1::2] if ids.count(v) > 1][:30]
    assert len(left_out) == 30
    for v in left_out:
        skip[ids.index(v)] = 0
    selects.append(skip)
    selects.append(np.zeros(1000, np.uint8))
    for sel in selects:
        order = np.arange(1000) if sel is None else np.nonzero(sel)[0]
        want = first_occurrences(a, order, known)
        got = dx.first_new(a, sel).cpu().numpy()
        assert got.dtype == bool and (got == want).all(), np.nonzero(got != want)[0][:10]
        if sel is None or sel.any():
            assert want.any()
    # against an empty set too (nothing known)
    empty = DeviceIndex(0)
    assert (empty.first_new(a).cpu().numpy() == first_occurrences(a, np.arange(1000), set())).all()
    # n = 0 and n = 1
    assert dx.first_new(np.zeros((0, 32), np.uint8)).shape == (0,)
    assert dx.first_new(arr([values[1]])).cpu().tolist() == [True]
    assert dx.first_new(arr([values[0]])).cpu().tolist() == [False]
    assert dx.first_new(arr([values[1]]), np.zeros(1, np.uint8)).cpu().tolist() == [False]
    # a device tensor as input, and the index unchanged by all of it
    import torch
    got = dx.first_new(torch.from_numpy(a).cuda()).cpu().numpy()
    assert (got == first_occurrences(a, np.arange(1000), known)).all()
    assert (dx.lookup(DATA, arr(values)).cpu().numpy() == before).all()
    assert dx.size(DATA) == len(known) == dx.keys(DATA)
    dx.close()
    empty.close()


# ---- the reference's tests, restated ------------------------------------------

def _reference_packs():
    from rustic_core_amd.index import IndexBlob, IndexPack
    d = [sha("data blob", k) for k in range(5)]
    t = [sha("tree blob", k) for k in range(2)]
    packs = [
        IndexPack(sha("pack", 0), [IndexBlob(d[0], 0, 0, 2000, 5000),
                                   IndexBlob(d[1], 0, 2000, 3185, None),
                                   IndexBlob(d[2], 0, 5185, 2095, 6411)]),
        IndexPack(sha("pack", 1), [IndexBlob(d[3], 0, 0, 6324, 9000),
                                   IndexBlob(d[4], 0, 6324, 1413, 3752)]),
        IndexPack(sha("pack", 2), [IndexBlob(t[0], 1, 0, 794, 3030),
                                   IndexBlob(t[1], 1, 794, 592, 1912)]),
    ]
    return packs, d, t


@pytest.fixture(scope="module")
def ref_indexes():
    from rustic_core_amd import DeviceIndex, IndexType
    from rustic_core_amd.index import IndexFile
    packs, d, t = _reference_packs()
    files = [IndexFile(packs[:1], packs_to_delete=[packs[2]]), IndexFile(packs[1:])]
    out = {it: DeviceIndex.from_index_files(files, 0, it) for it in IndexType}
    yield out, packs, d, t
    for dx in out.values():
        dx.close()


def _none(dx, tpe, id_):
    assert not dx.has(tpe, id_) and dx.get_id(tpe, id_) is None


def test_ref_all_index_types(ref_indexes):
    from rustic_core_amd.dindex import DATA, TREE
    idx, packs, d, t = ref_indexes
    one_off = bytes([d[2][0] ^ 0x50]) + d[2][1:]   # one byte off a real data id
    for dx in idx.values():
        for id_ in (b"\x00" * 32, one_off):
            _none(dx, DATA, id_)
            _none(dx, TREE, id_)
        _none(dx, DATA, t[1])                        # a tree id asked as data
        assert dx.has(TREE, t[1])
        pack, b = dx.get_id(TREE, t[1])
        assert pack == packs[2].id
        assert (b.id, b.type, b.offset, b.length, b.uncompressed_length) == (t[1], 1, 794, 592,
                                                                            1912)
        assert dx.total_size(TREE) == packs[2].pack_size() == 794 + 592 + 2 * 41 + 36
        assert dx.total_size(DATA) == packs[0].pack_size() + packs[1].pack_size()
        assert dx.packs(TREE) == [packs[2].id] and dx.packs(DATA) == [packs[0].id, packs[1].id]


def test_ref_only_trees(ref_indexes):
    from rustic_core_amd import IndexType
    from rustic_core_amd.dindex import DATA, TREE
    idx, packs, d, t = ref_indexes
    dx = idx[IndexType.ONLY_TREES]
    for id_ in (d[2], d[4]):
        _none(dx, DATA, id_)
        _none(dx, TREE, id_)
    assert len(dx) == 2
    assert not dx.has(DATA, arr(d)).cpu().numpy().any()


def test_ref_full_trees(ref_indexes):
    from rustic_core_amd import IndexType
    from rustic_core_amd.dindex import DATA, TREE
    idx, packs, d, t = ref_indexes
    dx = idx[IndexType.DATA_IDS]
    for id_ in (d[2], d[4]):
        assert dx.has(DATA, id_) and dx.get_id(DATA, id_) is None
        _none(dx, TREE, id_)
    assert len(dx) == 7
    assert dx.has(DATA, arr(d + t)).cpu().tolist() == [True] * 5 + [False] * 2


def test_ref_full(ref_indexes):
    from rustic_core_amd import IndexType
    from rustic_core_amd.dindex import DATA, TREE
    idx, packs, d, t = ref_indexes
    dx = idx[IndexType.FULL]
    for id_, pack, loc in ((d[2], packs[0].id, (5185, 2095, 6411)),
                           (d[4], packs[1].id, (6324, 1413, 3752)),
                           (d[1], packs[0].id, (2000, 3185, None))):   # None against a value
        assert dx.has(DATA, id_)
        p, b = dx.get_id(DATA, id_)
        assert p == pack and (b.offset, b.length, b.uncompressed_length) == loc and b.type == 0
        assert dx.get(id_) == (p, b)
        _none(dx, TREE, id_)
    assert dx.get(t[0]) is None and dx.get(b"\x00" * 32) is None
    got = dx.entries(DATA, [d[4], t[0], d[0]])
    assert got[1] is None and got[0][0] == packs[1].id and got[2][1].uncompressed_length == 5000
    assert len(dx) == 7 and dx.size(DATA) == 5 and dx.size(TREE) == 2


# ---- refused on the count alone -------------------------------------------------

def test_add_past_the_entry_limit_is_refused(raw):
    """size + n >= 2^32 - 1 is InvalidInput before anything is read: the
    buffers hold 64 bytes."""
    small = np.zeros(64, np.uint8)
    raw.add([sha("held")], [(1, 2, 3, 4)])
    for n in (0xFFFFFFFE, 0xFFFFFFFF, 1 << 40, (1 << 64) - 1):   # size is 1: 1 + n >= 2^32 - 1
        assert raw.L.rcdc_dindex_add(raw.h, small.ctypes.data, small.ctypes.data, n, 0, None) == 2
        assert "2^32" in raw._lib.last_error()
    assert raw.L.rcdc_dindex_add(raw.h, small.ctypes.data, None, 1, 2, None) == 2   # flag bits
    assert raw.L.rcdc_dindex_add(raw.h, None, None, 1, 0, None) == 2                # null ids
    assert raw.L.rcdc_dindex_lookup(raw.h, None, 1, None, None) == 2
    assert raw.L.rcdc_dindex_first_new(raw.h, None, 1, None, None, None) == 2
    assert raw.size() == 1
    raw.check([sha("held")] + ABSENT[:10])
