"""``repair snapshots`` on the device: rcdc_repair_trees_level and
rcdc_repair_spread against the numpy models (tests/repair_model.py),
``repair.plan_repair(device=0)`` against ``device=None`` on the built
repositories (tests/repair_repo.py) and the reference's recorded ones, and
``apply_repair``: the repaired repository goes through the project's check."""
import hashlib
import json
import types

import numpy as np
import pytest

from oracle import oracle, zstd_ref as zr
from tests import repair_model as model
from tests import repair_repo as rr
from tests import tree_nodes_model as tnm
from tests.check_cases import REPOS, Repo
from tests.check_trees_repo import Packed

pytestmark = pytest.mark.gpu

GUARD = 64
F, D = 0, 1
NO = model.NO_EDGE


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _hits(x, id_only: bool):
    """(n, 2) of (count, pack) -- or (count, entry) of an id-only set -- as
    (n, 6) int32 hit records."""
    x = np.asarray(x, np.int64).reshape(-1, 2)
    rec = np.zeros((len(x), 6), np.int64)
    if id_only:
        rec[:, 0], rec[:, 1], rec[:, 2] = x[:, 1], x[:, 0], NO
    else:
        rec[:, 0], rec[:, 1], rec[:, 2] = np.where(x[:, 0] != 0, 0, NO), x[:, 0], x[:, 1]
    return _up(rec.astype(np.uint32).view(np.int32))


def run_level(nodes, data_hits, tree_hits, is_dir, blob_slot, n_slots, before=None):
    """The level kernel against the model: the edges and the guard behind
    them, every byte of ``damaged`` and the guard behind it, the counts."""
    import torch
    from rustic_core_amd.repair import run_repair_level
    nodes = tnm.node_array(nodes) if isinstance(nodes, list) else nodes
    want_damaged, want_edges, want_counts = model.level_model(nodes, data_hits, tree_hits, is_dir,
                                                              blob_slot, n_slots)
    res = types.SimpleNamespace(node_records=_up(nodes.view(np.uint8).reshape(-1, 32).copy()),
                                tree_is_dir=_up(np.asarray(is_dir, np.uint8)))
    start = np.zeros(n_slots, np.uint8) if before is None else np.asarray(before, np.uint8).copy()
    flat = torch.full((n_slots + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    flat[:n_slots] = _up(start)
    edges, r = run_repair_level(res, _hits(data_hits, False), _hits(tree_hits, True),
                                _up(np.asarray(blob_slot, np.int64).astype(np.uint32).view(np.int32)),
                                flat[:n_slots], guard=GUARD)
    m = len(want_edges)
    got = edges.cpu().numpy()
    assert len(got) == m * 8 + GUARD and (got[m * 8:] == 0xA5).all()
    assert np.array_equal(got[:m * 8].view(np.uint32).reshape(m, 2), want_edges)
    after = flat.cpu().numpy()
    assert (after[n_slots:] == 0xA5).all()
    want = start.copy()
    want[want_damaged] = 1
    assert np.array_equal(after[:n_slots], want)
    assert (int(r.missing_ids), int(r.damaged_nodes), int(r.files_without_content),
            int(r.first_without_content)) == want_counts
    return want_damaged, want_edges, want_counts


def _random_level(n_nodes: int, n_blobs: int, seed: int, p_missing=0.1, no_content=False):
    """Every node type with and without a subtree, files of 0 to 3 ids
    between each other, ``n_blobs`` blobs of about the same size."""
    rng = np.random.default_rng(seed)
    nodes, data_hits, tree_hits, is_dir = [], [], [], []
    n_slots = n_blobs + 40
    for k in range(n_nodes):
        tpe = int(rng.choice([F, F, F, D, D, 2, 3, 4, 5, 6]))
        has_sub = bool(rng.random() < (0.8 if tpe == D else 0.3))
        content = tpe == F and not (no_content and rng.random() < 0.2)
        n_ids = int(rng.choice([0, 0, 1, 2, 3])) if (content or (tpe != F and rng.random() < 0.3)) else 0
        flags = (model.CONTENT if content or (tpe != F and n_ids) else 0) | (model.SUBTREE if has_sub else 0)
        nodes.append((0, 0, k * n_blobs // max(n_nodes, 1), len(data_hits), n_ids, len(tree_hits), tpe,
                      flags, 0))
        if tpe == F:
            for _ in range(n_ids):
                u = rng.random()
                data_hits.append((0, 0) if u < p_missing else (1, NO) if u < 1.5 * p_missing
                                 else (int(rng.integers(1, 4)), int(rng.integers(0, 30))))
        if has_sub:
            tree_hits.append((1, int(rng.integers(0, n_slots))) if rng.random() < 0.9 else (0, NO))
            is_dir.append(int(tpe == D))
    return nodes, data_hits, tree_hits, is_dir, list(range(7, 7 + n_blobs)), n_slots


@pytest.mark.parametrize("n_nodes", (0, 1, 63, 64, 65, 257, 1025))
def test_level_node_counts(gpu_ctx, n_nodes):
    args = _random_level(n_nodes, max(1, n_nodes // 50), 100 + n_nodes)
    damaged, edges, counts = run_level(*args)
    if n_nodes >= 63:
        assert damaged and counts[0] and counts[1] and (edges[:, 0] != NO).any() \
            and (edges[:, 0] == NO).any()
    assert counts[2:] == (0, model.NO_NODE)


def test_level_every_type_with_and_without_subtree(gpu_ctx):
    nodes, tree_hits, is_dir = [], [], []
    for tpe in range(7):
        for sub in (False, True):
            nodes.append((0, 0, tpe % 3, 0, 0, len(tree_hits), tpe,
                          (model.CONTENT if tpe == F else 0) | (model.SUBTREE if sub else 0), 0))
            if sub:
                tree_hits.append((1, 20 + tpe))
                is_dir.append(int(tpe == D))
    damaged, edges, counts = run_level(nodes, [], tree_hits, is_dir, [3, 4, 5], 30)
    assert damaged == [4]                       # the dir without a subtree, in blob 1
    assert counts == (0, 1, 0, model.NO_NODE)
    assert [tuple(e) for e in edges.tolist()] == [(NO, NO), (4, 21)] + [(NO, NO)] * 5
    # a subtree the set lacks, a slot past the array, a blob past the slots: no edge, no store
    run_level([(0, 0, 0, 0, 0, 0, D, model.SUBTREE, 0), (0, 0, 1, 0, 0, 1, D, model.SUBTREE, 0),
               (0, 0, 2, 0, 0, 2, D, 0, 0), (0, 0, 9, 0, 0, 2, D, 0, 0)],
              [], [(0, NO), (1, 99)], [1, 1], [0, 1, 50], 10)


def test_level_ties_in_data_start(gpu_ctx):
    """Files with no ids between files with ids, and nodes of other types
    whose ids are not in d_data_ids: they share a data_start with their
    neighbour, and each missing id still finds its own node."""
    for miss in ((), (0,), (1,), (2,), (3,), (0, 1, 2, 3)):
        nodes = [(0, 0, 0, 0, 0, 0, F, 1, 0), (0, 0, 0, 0, 2, 0, F, 1, 0), (0, 0, 0, 2, 5, 0, 5, 1, 0),
                 (0, 0, 1, 2, 0, 0, F, 1, 0), (0, 0, 1, 2, 0, 0, F, 1, 0), (0, 0, 2, 2, 1, 0, F, 1, 0),
                 (0, 0, 3, 3, 0, 0, F, 1, 0), (0, 0, 4, 3, 1, 0, F, 1, 0), (0, 0, 5, 4, 0, 0, F, 1, 0)]
        hits = [(0, 0) if i in miss else (2, 5) for i in range(4)]
        damaged, _, counts = run_level(nodes, hits, [], [], [10, 11, 12, 13, 14, 15], 16)
        assert damaged == sorted({(10, 10, 12, 14)[i] for i in miss})
        assert counts[0] == len(miss)


@pytest.mark.parametrize("at", (0, 4095, 4096))
def test_level_a_file_of_4097_ids(gpu_ctx, at):
    """One lane per id: the one missing id of a long file at its first place,
    at the last of a block of 256 lanes times 16 and one past it."""
    nodes = [(0, 0, 0, 0, 1, 0, F, 1, 0), (0, 0, 1, 1, 4097, 0, F, 1, 0), (0, 0, 2, 4098, 1, 0, F, 1, 0)]
    hits = [(1, 3)] * 4099
    hits[1 + at] = (0, 0)
    damaged, _, counts = run_level(nodes, hits, [], [], [5, 6, 7], 8)
    assert damaged == [6] and counts == (1, 1, 0, model.NO_NODE)


@pytest.mark.parametrize("n_blobs", (1, 2, 257))
def test_level_damage_in_the_last_blob_only(gpu_ctx, n_blobs):
    nodes, hits = [], []
    for b in range(n_blobs):
        nodes.append((0, 0, b, len(hits), 2, 0, F, 1, 0))
        hits += [(1, 1), (1, 2)]
    hits[-1] = (0, 0)
    before = np.zeros(n_blobs + 3, np.uint8)
    before[0] = 1  # an earlier level's mark stays
    damaged, _, _ = run_level(nodes, hits, [], [], list(range(2, 2 + n_blobs)), n_blobs + 3, before)
    assert damaged == [n_blobs + 1]


def test_level_files_without_content(gpu_ctx):
    args = _random_level(700, 9, 5, no_content=True)
    _, _, counts = run_level(*args)
    assert counts[2] > 20 and counts[3] != model.NO_NODE
    nodes = [(0, 0, 0, 0, 0, 0, D, model.SUBTREE, 0)] * 300 + [(0, 0, 0, 0, 0, 0, F, 0, 0)] * 2
    nodes = [n[:5] + (i,) + n[6:] for i, n in enumerate(nodes)]
    _, _, counts = run_level(nodes, [], [(1, 1)] * 300, [1] * 300, [0], 4)
    assert counts == (0, 0, 2, 300)


# ---- the spread ------------------------------------------------------------------------------

def run_spread(edges, damaged):
    from rustic_core_amd.repair import run_repair_spread
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    damaged = np.asarray(damaged, np.uint8)
    flat, rounds = run_repair_spread(_up(edges.astype(np.uint32).view(np.int32)), _up(damaged),
                                     guard=GUARD)
    got = flat.cpu().numpy()
    assert len(got) == len(damaged) + GUARD and (got[len(damaged):] == 0xA5).all()
    want = model.spread_model(edges, damaged)
    assert np.array_equal(got[:len(damaged)], want)
    assert rounds <= len(damaged) + 1
    return want, rounds


def test_spread_small_graphs(gpu_ctx):
    want, rounds = run_spread([], [0, 1, 0])                                   # no edges
    assert want.tolist() == [0, 1, 0] and rounds == 0
    want, rounds = run_spread([(0, 1), (1, 2)], [0, 0, 0])                     # no damage
    assert not want.any() and rounds == 1
    want, _ = run_spread([(0, 1), (0, 2), (1, 3), (2, 3), (4, 0)], [0, 0, 0, 1, 0, 0])  # a diamond
    assert want.tolist() == [1, 1, 1, 1, 1, 0]
    # P (1) under the root (0) and again under R (3), Q (2) over R, the damage (4) below P
    want, _ = run_spread([(0, 1), (0, 2), (2, 3), (3, 1), (1, 4), (0, 5)], [0, 0, 0, 0, 1, 0])
    assert want.tolist() == [1, 1, 1, 1, 1, 0]
    want, rounds = run_spread([(0, 1), (1, 2), (2, 0), (3, 0), (1, 4)], [0, 0, 1, 0, 0])  # a cycle
    assert want.tolist() == [1, 1, 1, 1, 0] and rounds >= 2
    want, rounds = run_spread([(NO, NO)] * 700, [0, 1, 0])                     # all NO_EDGE
    assert want.tolist() == [0, 1, 0] and rounds == 1


def test_spread_a_chain_of_300(gpu_ctx):
    """The damage at the bottom: every ancestor changes, over more rounds
    than one launch holds."""
    from rustic_core_amd.repair import spread_rounds_per_launch
    want, rounds = run_spread([(i, i + 1) for i in range(299)], [0] * 299 + [1])
    assert want.all()
    assert rounds >= 300 / spread_rounds_per_launch() and rounds > spread_rounds_per_launch()


def test_spread_a_random_dag(gpu_ctx):
    """2^18 + 5 edges over 2^16 slots: more than one workgroup per round by
    far, parents and children anywhere."""
    rng = np.random.default_rng(11)
    n, m = 1 << 16, (1 << 18) + 5
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    edges = np.stack([np.minimum(a, b), np.maximum(a, b)], 1)  # parent < child, or a self loop
    damaged = np.zeros(n, np.uint8)
    damaged[rng.integers(n - 2000, n, 3)] = 1
    want, rounds = run_spread(edges, damaged)
    assert 100 < int(want.sum()) < n and rounds >= 2


# ---- plans: the device against the host ----------------------------------------------------------

_PACKED = {}


class Built:
    """tests/repair_repo.py's repository packed on the device, with sealed
    snapshot files."""

    def __init__(self, gpu_ctx, no_content=False):
        self.p = Packed(gpu_ctx, rr.build(no_content=no_content))
        self.snapshots = []
        for n, t in enumerate(self.p.repo.snapshots):
            sealed = self.p.key.encrypt_data(rr.snapshot_file(t, n), bytes([n + 1]) * 16)
            self.snapshots.append((hashlib.sha256(sealed).digest(), sealed))

    def without(self, *names):
        return [self.p.names[n] for n in names]

    def plans(self, snapshots=None, without=("lostleaf",), budget=1 << 30, opts=None):
        from rustic_core_amd.repair import RepairSnapshotsOptions, plan_repair
        opts = opts or RepairSnapshotsOptions()
        snaps = self.snapshots if snapshots is None else snapshots
        lack = self.without(*without)
        dx = self.p.index(lack)
        try:
            dev = plan_repair(self.p.key, dx, snaps, self.p.reader(), opts, device=0, budget=budget)
        finally:
            dx.close()
        host = plan_repair(self.p.key, self.p.host_index(lack), snaps, self.p.reader(), opts,
                           device=None, decode=zr.decompress)
        return dev, host


def _built(gpu_ctx, no_content=False) -> Built:
    if no_content not in _PACKED:  # built once for the module, never changed
        _PACKED[no_content] = Built(gpu_ctx, no_content)
    return _PACKED[no_content]


def _same(dev, host):
    for a, b in zip(dev.fields(), host.fields()):
        assert a == b
    assert len(dev.fields()) == 5


def test_built_repository_device_against_host(gpu_ctx):
    b = _built(gpu_ctx)
    dev, host = b.plans()
    _same(dev, host)
    name = lambda t: b.p.repo.names.get(t, "empty")
    assert {name(t) for t in dev.changed} == {
        "nosub", "zero", "twin1", "twin2", "already", "sizefix", "lostleaf", "keeps", "rules",
        "backleaf", "P", "R", "Q", "backroot", "hostbelow", "host", "hostroot"}
    assert [s.new_tree is not None for s in dev.snapshots] == [True, True, False, False, True]
    # the tree outside the grammar during the walk; then the 19 marked trees of which two are lost
    assert dev.stats["host_parsed_blobs"] == 1 + 17
    marked = set(dev.changed) | {b.p.names["sameid"]}
    assert dev.stats["text_bytes_to_host"] == len(b.p.repo.trees[b.p.names["host"]]) + \
        sum(len(b.p.repo.trees[t]) for t in marked if t != b.p.names["lostleaf"])
    assert dev.stats["spread_rounds"] >= 2
    # one group per blob: the same plan
    small, _ = b.plans(budget=1)
    _same(small, host)
    # other options
    from rustic_core_amd.repair import RepairSnapshotsOptions
    _same(*b.plans(opts=RepairSnapshotsOptions(delete=False, suffix="~", tags=("x,y",))))


def test_a_file_without_content_raises_on_both_routes(gpu_ctx):
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.repair import plan_repair
    b = _built(gpu_ctx, no_content=True)
    dx = b.p.index()
    msgs = []
    for device, index, decode in ((0, dx, None), (None, b.p.host_index(), zr.decompress)):
        with pytest.raises(RusticError) as e:
            plan_repair(b.p.key, index, b.snapshots, b.p.reader(), device=device, decode=decode)
        assert e.value.kind == ErrorKind.Internal
        msgs.append(str(e.value))
    dx.close()
    assert msgs[0] == msgs[1] and '`a/b"q/nc`' in msgs[0]


def test_a_clean_repository_stays_on_the_device(gpu_ctx, monkeypatch):
    """Nothing to repair inside the grammar: no text crosses -- the host
    parsers are not even callable."""
    from rustic_core_amd import repair, tree
    from rustic_core_amd.repair import plan_repair
    b = _built(gpu_ctx)
    snaps = b.snapshots[2:4]  # cleanroot and oddroot
    host = plan_repair(b.p.key, b.p.host_index(), snaps, b.p.reader(), device=None,
                       decode=zr.decompress)

    def never(text):
        raise AssertionError("a tree blob's text reached the host parser")
    monkeypatch.setattr(repair, "parse_tree_full", never)
    monkeypatch.setattr(tree, "parse_tree_nodes_host", never)
    dx = b.p.index()
    dev = plan_repair(b.p.key, dx, snaps, b.p.reader(), device=0)
    dx.close()
    _same(dev, host)
    assert dev.changed == {} and dev.new_trees == [] and dev.delete == [] and len(dev.unchanged) == 5
    assert dev.stats == {"text_bytes_to_host": 0, "host_parsed_blobs": 0, "spread_rounds": 1}


@pytest.mark.parametrize("name", REPOS)
def test_recorded_repositories_device_against_host(gpu_ctx, name):
    from rustic_core_amd.check import HostIndex, _decrypt_file
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.dindex import DeviceIndex
    from rustic_core_amd.index import IndexFile
    from rustic_core_amd.repair import plan_repair
    repo = Repo(name, oracle)
    k = Key(repo.master)
    files = [IndexFile.from_json(_decrypt_file(k, repo.read_full("index", i), 0, None))
             for i, _ in repo.list_with_size("index")]
    packs = [p for f in files for p in f.packs]
    snaps = sorted(repo.by_type["snapshot"].items())
    dx = DeviceIndex(0)
    dx.extend(packs)
    try:
        dev = plan_repair(k, dx, snaps, repo.read_partial, device=0)
    finally:
        dx.close()
    host = plan_repair(k, HostIndex(packs), snaps, repo.read_partial, device=None,
                       decode=zr.decompress)
    _same(dev, host)
    damaged = name in ("repo-index-missing-blob.tar.gz", "repo-index-missing.tar.gz", "repo-mixed.tar.gz")
    assert bool(dev.changed) == damaged
    if not damaged:
        assert dev.stats["text_bytes_to_host"] == 0 and dev.stats["host_parsed_blobs"] == 0


# ---- apply ------------------------------------------------------------------------------------------

_KINDS = ("FileBlobNotInIndex", "FileBlobHasNullId", "NoSubTree", "SubTreeMissingInIndex")


def _blobs_of(pack: bytes, index_pack, open_):
    """{id: plain text} of a new pack: every blob opened and decoded, and the
    header against the index entries."""
    from rustic_core_amd.pack import parse_header
    hlen = int.from_bytes(pack[-4:], "little")
    header = parse_header(open_(pack[-4 - hlen:-4]))
    assert [(e.id, e.type, e.offset, e.length, e.uncompressed_len or None) for e in header] == \
        [(b.id, b.type, b.offset, b.length, b.uncompressed_length) for b in index_pack.blobs]
    out = {}
    for b in index_pack.blobs:
        plain = open_(pack[b.offset:b.offset + b.length])
        out[b.id] = zr.decompress(plain) if b.uncompressed_length else plain
        assert b.type == 1 and hashlib.sha256(out[b.id]).digest() == b.id
    return out


def _applied(plan, result, open_):
    """What apply_repair returned, on the host: the packs' blobs are the
    planned texts, the snapshot files open to the planned texts."""
    new_packs = {p.id: p.data.cpu().numpy().tobytes() for p in result.packs}
    assert all(hashlib.sha256(v).digest() == i for i, v in new_packs.items())
    blobs = {}
    for p in result.packs:
        blobs.update(_blobs_of(new_packs[p.id], p.index, open_))
    assert blobs == dict(plan.new_trees) and result.tree_ids == [i for i, _ in plan.new_trees]
    snaps = {i: t.cpu().numpy().tobytes() for i, t in result.snapshots}
    assert all(hashlib.sha256(v).digest() == i for i, v in snaps.items())
    texts = []
    for v in snaps.values():
        plain = open_(v)
        texts.append(zr.decompress(plain[1:]) if plain[:1] == b"\x02" else plain)
    assert texts == [s.text for s in plan.snapshots if s.text is not None]
    index_files = {i: t.cpu().numpy().tobytes() for i, t in result.index_files}
    assert all(hashlib.sha256(v).digest() == i for i, v in index_files.items())
    assert result.delete == plan.delete
    return new_packs, index_files, snaps


def test_apply_on_repo_index_missing_blob(gpu_ctx):
    """The reference's test of this command: after the repair, check with
    read_data is ok."""
    from rustic_core_amd.check import _decrypt_file, check_repository
    from rustic_core_amd.chunker import ConfigFile
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.dindex import DeviceIndex
    from rustic_core_amd.errors import RusticError
    from rustic_core_amd.index import IndexFile
    from rustic_core_amd.repair import repair_snapshots
    from rustic_core_amd.tree import snapshot_trees
    repo = Repo("repo-index-missing-blob.tar.gz", oracle)
    k = Key(repo.master)
    cfg = json.loads(k.decrypt_data(repo.files["repo/config"]))
    config = ConfigFile(version=int(cfg["version"]), compression=cfg.get("compression"))
    check = lambda r: check_repository(k, r.list_with_size, r.read_full, r.read_partial,
                                       snapshot_trees(k, r.snapshots(), device=0), read_data=True,
                                       device=0)
    with pytest.raises(RusticError):
        check(repo).is_ok()
    files = [IndexFile.from_json(_decrypt_file(k, repo.read_full("index", i), 0, None))
             for i, _ in repo.list_with_size("index")]
    snaps = sorted(repo.by_type["snapshot"].items())
    dx = DeviceIndex(0)
    dx.extend([p for f in files for p in f.packs])
    try:
        plan, result = repair_snapshots(k, dx, snaps, repo.read_partial, config)
        _, dry = repair_snapshots(k, dx, snaps, repo.read_partial, config, dry_run=True)
    finally:
        dx.close()
    assert dry.tree_ids == result.tree_ids and dry.delete == result.delete == [snaps[0][0]]
    assert dry.packs == [] and dry.index_files == [] and dry.snapshots == []
    assert len(result.tree_ids) == 4 and len(result.snapshots) == 1 and len(result.index_files) == 1
    new_packs, index_files, new_snaps = _applied(plan, result, lambda b: oracle.open_(repo.master, b))
    # the repaired repository: the old files, plus the new, minus the deleted snapshot
    repo.by_type["pack"].update(new_packs)
    repo.by_type["index"].update(index_files)
    repo.by_type["snapshot"].update(new_snaps)
    for i in result.delete:
        del repo.by_type["snapshot"][i]
    got = check(repo)
    got.is_ok()
    assert not [f for _, f in got if f.kind in _KINDS + ("ErrorCheckingTrees",)]


def test_apply_on_the_built_repository(gpu_ctx):
    from rustic_core_amd.check import check_trees
    from rustic_core_amd.chunker import ConfigFile
    from rustic_core_amd.dindex import DeviceIndex
    from rustic_core_amd.index import IndexFile
    from rustic_core_amd.repair import repair_snapshots
    from rustic_core_amd.restore import from_packs
    b = _built(gpu_ctx)
    p = b.p
    lack = b.without("lostleaf")
    snaps = b.snapshots[:3] + b.snapshots[4:]  # not the tree under a symlink, which check follows
    dx = p.index(lack)
    try:
        plan, result = repair_snapshots(p.key, dx, snaps, p.reader(), ConfigFile(version=2))
        _, dry = repair_snapshots(p.key, dx, snaps, p.reader(), ConfigFile(version=2), dry_run=True)
    finally:
        dx.close()
    assert dry.tree_ids == result.tree_ids and dry.delete == result.delete and dry.packs == []
    new_packs, index_files, _ = _applied(plan, result, p.key.decrypt_data)
    assert len(result.snapshots) == 3 and len(result.packs) >= 1
    # the index files hold the new packs
    listed = [ip for v in index_files.values()
              for ip in IndexFile.from_json(zr.decompress(p.key.decrypt_data(v)[1:])).packs]
    assert sorted(ip.id for ip in listed) == sorted(new_packs)
    # the repaired repository through check_trees
    roots = [s.new_tree or s.tree for s in plan.snapshots]
    before = DeviceIndex.from_index_files([IndexFile(p.index_packs(lack))])
    after = DeviceIndex.from_index_files([IndexFile(p.index_packs(lack) + listed)])
    reader = from_packs({**p.packs, **new_packs})
    try:
        findings = []
        with pytest.raises(Exception):
            check_trees(p.key, before, [s.tree for s in plan.snapshots], reader, findings=findings)
        assert {f.kind for _, f in findings} >= {"FileBlobNotInIndex", "NoSubTree"}
        got, _ = check_trees(p.key, after, roots, reader)
    finally:
        before.close()
        after.close()
    assert not [f for _, f in got if f.kind in _KINDS]
