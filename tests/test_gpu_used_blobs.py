"""tree.find_used_blobs on the device against the plain-Python walk
(``device=None``) and against the walk written over the objects
(tests/used_blobs_repo.py): the reference's own repository (repo-mixed
fixture) and a repository built with the project's packer and sealing."""
import hashlib

import numpy as np
import pytest

from oracle import oracle
from tests.test_gpu_pack import _build
from tests.test_gpu_read import _dev
from tests.test_gpu_zstd_check import _device_frames
from tests.test_used_blobs_host import fixture, rows
from tests.used_blobs_repo import build, did, walk

pytestmark = pytest.mark.gpu

KEY = bytes(range(64))


def _rows(t):
    return rows(t.cpu().numpy())


def test_reference_repository(gpu_ctx):
    """repo-mixed: its snapshot's tree, its index, its pack.  The pack mixes
    a data blob and four tree blobs, and the collector files a pack under
    the type of its first blob (binarysorted.rs:127-163), so get_tree finds
    nothing of it; here its blobs are indexed as one pack per type."""
    from rustic_core_amd import DeviceIndex
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.index import IndexFile, IndexPack
    from rustic_core_amd.read import read_blobs
    from rustic_core_amd.restore import from_packs
    from rustic_core_amd.tree import OK, find_used_blobs, parse_trees, snapshot_trees
    key, files, index_file, pack_id = fixture(oracle)
    k = Key(key)
    sealed = [v for n, v in files.items() if n.startswith("repo/snapshots/")]
    trees = snapshot_trees(k, sealed)
    assert len(trees) == 1
    whole = index_file.packs[0]
    split = [IndexPack(whole.id, [b for b in whole.blobs if b.type == t]) for t in (0, 1)]
    assert [len(p.blobs) for p in split] == [1, 4]
    dx = DeviceIndex.from_index_files([IndexFile(split)])
    pack = [v for n, v in files.items() if n.startswith("repo/data/")][0]
    used = find_used_blobs(k, dx, trees, from_packs({pack_id: pack}))
    host = find_used_blobs(k, dx, trees, from_packs({pack_id: pack}), device=None)
    assert _rows(used) == rows(host) and len(host) == 5
    assert sorted(rows(host)) == sorted(b.id for b in whole.blobs) and rows(host)[0] == trees[0]
    # the reference's own bytes: every tree blob of the fixture is in G_T
    plain = read_blobs(k, _dev(pack), split[1].blobs)
    res = parse_trees(plain.data, plain.offsets, plain.lengths)
    assert res.blobs["status"].tolist() == [OK] * 4
    assert res.nodes == 4 and res.n_tree_ids == 3 and res.n_data_ids == 1
    dx.close()


class Built:
    """The repository of used_blobs_repo.build() in three tree packs made by
    the device packer, every third tree blob a zstd frame of the device
    encoder."""

    def __init__(self, gpu_ctx, broken=None):
        from rustic_core_amd.crypto import Key
        from rustic_core_amd.index import IndexPack
        from rustic_core_amd.pack import parse_header
        self.repo = r = build()
        self.names = {v: k for k, v in r.names.items()}
        rng = np.random.default_rng(5)
        ids = list(r.trees)
        texts = [r.trees[i] for i in ids]
        if broken is not None:  # that tree's text cut short: no JSON, still its id in the index
            texts[ids.index(broken)] = texts[ids.index(broken)][:-3]
        comp = [n % 3 == 0 for n in range(len(ids))]
        frames = iter(_device_frames(gpu_ctx, [t for t, c in zip(texts, comp) if c]))
        datas = [next(frames) if c else t for t, c in zip(texts, comp)]
        specs = [(1, np.frombuffer(i, np.uint8), bytes(rng.integers(0, 256, 16, dtype=np.uint8)),
                  len(t) if c else 0) for i, t, c in zip(ids, texts, comp)]
        groups = [(0, 13), (13, 13), (26, 14)]
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
        assert sum(1 for p in self.index_packs for b in p.blobs if b.uncompressed_length) == 14

    def index(self, without=()):
        from rustic_core_amd import DeviceIndex
        from rustic_core_amd.index import IndexFile, IndexPack
        packs = [IndexPack(p.id, [b for b in p.blobs if b.id not in without])
                 for p in self.index_packs]
        return DeviceIndex.from_index_files([IndexFile(packs)])

    def reader(self):
        from rustic_core_amd.restore import from_packs
        inner, calls = from_packs(self.packs), []

        def read_partial(pack_id, offset, length):
            calls.append((bytes(pack_id), offset, length))
            return inner(pack_id, offset, length)
        return read_partial, calls


_BUILT = {}


@pytest.fixture
def built(gpu_ctx):
    if "b" not in _BUILT:  # one repository for the whole module, never changed
        _BUILT["b"] = Built(gpu_ctx)
    return _BUILT["b"]


def test_built_repository(built):
    from rustic_core_amd.tree import find_used_blobs
    r = built.repo
    want, levels = walk(r)
    dx = built.index()
    read_partial, calls = built.reader()
    used = find_used_blobs(built.key, dx, r.snapshots, read_partial)
    assert str(used.device) == "cuda:0" and tuple(used.shape) == (97, 32)
    got = _rows(used)
    assert len(set(got)) == len(got)                      # distinct
    assert got == want                                    # the order as specified
    assert got[:3] == r.snapshots and got[3] == did("r0.0")
    # neighbours in a pack are read together: far fewer reads than trees, each tree once
    assert len(calls) < 40 and sum(c[2] for c in calls) <= sum(len(p) for p in built.packs.values())
    host = find_used_blobs(built.key, dx, r.snapshots, built.reader()[0], device=None)
    assert rows(host) == want                              # device == Python
    assert built.names["hidden"] not in got and did("hidden.0") in got
    assert built.names["mid7"] in got and did("m7.0") in got   # the NOT_PARSED tree and its children
    # a budget that forces one group per blob
    read_partial, calls = built.reader()
    assert _rows(find_used_blobs(built.key, dx, r.snapshots, read_partial, budget=1)) == want
    # a repeated snapshot tree, one snapshot, none
    assert _rows(find_used_blobs(built.key, dx, r.snapshots[::-1] + r.snapshots, read_partial)) == \
        walk(r, r.snapshots[::-1])[0]
    assert _rows(find_used_blobs(built.key, dx, r.snapshots[2:], read_partial)) == \
        walk(r, r.snapshots[2:])[0]
    assert tuple(find_used_blobs(built.key, dx, [], read_partial).shape) == (0, 32)
    dx.close()


def test_the_host_tree_is_not_parsed_on_the_device(built):
    """mid7 carries a key Node does not know: NOT_PARSED on the device, a
    tree for the host rule; every other tree of the repository is OK."""
    from rustic_core_amd.tree import NOT_PARSED, parse_trees
    from tests.test_gpu_tree_parse import _arena
    ids = list(built.repo.trees)
    d, offs, lens = _arena([built.repo.trees[i] for i in ids], align=16)
    st = parse_trees(d, offs, lens).blobs["status"].tolist()
    assert [ids[i] for i, s in enumerate(st) if s == NOT_PARSED] == [built.names["mid7"]]


def test_used_ids_feed_the_prune_plan(built):
    """find_used_blobs' device tensor is PrunePlan.from_entries' used_ids; the
    plan is the one the host-found ids give."""
    from rustic_core_amd.index import IndexFile, IndexPack
    from rustic_core_amd.prune import PruneOptions, PrunePack, PrunePlan
    from rustic_core_amd.tree import find_used_blobs
    from tests.prune_cases import CONFIG, NOW, bid, existing_of, plan_summary
    r = built.repo
    dx = built.index()
    used = find_used_blobs(built.key, dx, r.snapshots, built.reader()[0])
    host = find_used_blobs(built.key, dx, r.snapshots, built.reader()[0], device=None)
    dx.close()
    # data packs by name only: the used data blobs in packs of 7, and blobs no snapshot uses
    data_ids = [i for i in rows(host) if i not in r.trees] + [did(f"unused{i}") for i in range(9)]
    data_packs = []
    for p in range(0, len(data_ids), 7):
        ip = IndexPack(bid(f"datapack{p}"))
        for n, i in enumerate(data_ids[p:p + 7]):
            ip.add(i, 0, 100 * n, 68 + n, 200 if n % 2 else None)
        data_packs.append(ip)
    files = [(bid("index:0"), IndexFile(built.index_packs[:2] + data_packs[:3])),
             (bid("index:1"), IndexFile(built.index_packs[2:] + data_packs[3:]))]
    ids, lens, ulens, offs, recs = [], [], [], [], []
    for fno, (_, f) in enumerate(files):
        for p in f.packs:
            recs.append(PrunePack(p.id, p.blobs[0].type, p.pack_size(), p.time, False, fno,
                                  len(lens), len(p.blobs)))
            for b in p.blobs:
                ids.append(b.id)
                lens.append(b.length)
                ulens.append(b.uncompressed_length or 0)
                offs.append(b.offset)
    arrays = (np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32), np.array(lens, np.uint32),
              np.array(ulens, np.uint32), np.array(offs, np.uint32))
    opts = PruneOptions(max_unused="0%", max_repack="unlimited")
    plans = [plan_summary(PrunePlan.from_entries(*arrays, recs, [i for i, _ in files], u,
                                                 existing_of(files), opts, CONFIG, NOW, device=0))
             for u in (used, host)]
    assert plans[0] == plans[1]
    # hidden and the nine unused data blobs are the only blobs no snapshot uses
    assert sum(plans[0]["used"]) == len(ids) - 10


def test_errors(built, gpu_ctx):
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.tree import DESERIALIZE_MESSAGE, find_used_blobs
    r = built.repo
    # a subtree the index lacks
    leaf = built.names["leaf9"]
    dx = built.index(without=(leaf,))
    for device in (0, None):
        with pytest.raises(RusticError) as e:
            find_used_blobs(built.key, dx, r.snapshots, built.reader()[0], device=device)
        assert e.value.kind == ErrorKind.Internal
        assert f"Tree ID `{leaf.hex()}` not found in index" in str(e.value)
    dx.close()
    # a snapshot tree the index lacks
    dx = built.index()
    with pytest.raises(RusticError) as e:
        find_used_blobs(built.key, dx, [did("no tree")], built.reader()[0])
    assert "not found in index" in str(e.value)
    dx.close()
    # a tree blob that is not JSON
    bad = Built(gpu_ctx, broken=built.names["mid3"])
    dx = bad.index()
    for device in (0, None):
        with pytest.raises(RusticError) as e:
            find_used_blobs(bad.key, dx, r.snapshots, bad.reader()[0], device=device)
        assert e.value.kind == ErrorKind.Internal and DESERIALIZE_MESSAGE in str(e.value)
    dx.close()
