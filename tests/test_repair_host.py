"""CPU: trees and snapshots written on the host (rustic_core_amd/tree_write.py),
``repair.plan_repair(device=None)`` on the reference's recorded repositories
and on built ones (tests/repair_repo.py), the numpy models of the device
verdict (tests/repair_model.py) against that rule, and the argument checks of
rcdc_repair_trees_level and rcdc_repair_spread without a device."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from tests import repair_model as model
from tests import repair_repo as rr
from tests import tree_nodes_model as tnm
from tests.check_cases import REPOS, Repo
from tests.test_used_blobs_host import OracleKey

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                     "repair_snapshots.json")))
DAMAGED = ("repo-index-missing-blob.tar.gz", "repo-index-missing.tar.gz")
SYMBOLS = ("rcdc_repair_trees_level", "rcdc_repair_spread", "rcdc_repair_spread_rounds_per_launch")
T = "2020-02-22T20:58:54.199240159+01:00"


# ---- the recorded repositories ------------------------------------------------------------

class Recorded:
    """A fixture opened for the host route."""

    def __init__(self, name, oracle_mod):
        from oracle import zstd_ref as zr
        from rustic_core_amd.check import HostIndex, _decrypt_file
        from rustic_core_amd.index import IndexFile
        self.repo = Repo(name, oracle_mod)
        self.key = OracleKey(oracle_mod, self.repo.master)
        self.decode = zr.decompress
        files = [IndexFile.from_json(_decrypt_file(self.key, self.repo.read_full("index", i), None,
                                                   self.decode))
                 for i, _ in self.repo.list_with_size("index")]
        self.packs = [p for f in files for p in f.packs]
        self.index = HostIndex(self.packs)
        self.snapshots = sorted(self.repo.by_type["snapshot"].items())

    def tree_texts(self):
        """{id: text} of every tree blob the index holds and a pack gives."""
        from rustic_core_amd.repair import _HostLookups
        from rustic_core_amd.tree import _host_blob
        out = {}
        for p in self.packs:
            for b in p.blobs:
                if b.type == 1 and b.id not in out:
                    try:
                        out[b.id] = _host_blob(self.key, _HostLookups(self.index), b.id,
                                               self.repo.read_partial, self.decode, None)
                    except Exception:
                        pass  # filed under a data pack, or its pack is cut short
        return out

    def plan(self, opts=None):
        from rustic_core_amd.repair import RepairSnapshotsOptions, plan_repair
        return plan_repair(self.key, self.index, self.snapshots, self.repo.read_partial,
                           opts or RepairSnapshotsOptions(), device=None, decode=self.decode)


_RECORDED = {}


def recorded(name, oracle_mod) -> Recorded:
    if name not in _RECORDED:  # opened once, never changed
        _RECORDED[name] = Recorded(name, oracle_mod)
    return _RECORDED[name]


def test_the_32_fixture_trees_come_back_byte_for_byte(oracle_mod):
    from rustic_core_amd.tree_write import parse_tree_full, serialize_tree
    n = 0
    for name in REPOS:
        for tid, text in recorded(name, oracle_mod).tree_texts().items():
            assert hashlib.sha256(text).digest() == tid
            assert serialize_tree(parse_tree_full(text)) == (text, tid), (name, tid.hex())
            n += 1
    assert n == 32


def test_plan_on_repo_index_missing_blob(oracle_mod):
    """One snapshot, changed.  The new ids by text surgery on the four known
    tree texts: the leaf's file loses its one blob, each ancestor gets the new
    subtree."""
    r = recorded("repo-index-missing-blob.tar.gz", oracle_mod)
    texts = r.tree_texts()
    assert len(texts) == 4 and len(r.snapshots) == 1
    sid, sealed = r.snapshots[0]
    snap = json.loads(r.key.decrypt_data(sealed))
    chain = [bytes.fromhex(snap["tree"])]  # root, home, thinkpad, data
    while True:
        nodes = json.loads(texts[chain[-1]])["nodes"]
        if nodes[0]["type"] != "dir":
            break
        assert len(nodes) == 1
        chain.append(bytes.fromhex(nodes[0]["subtree"]))
    assert len(chain) == 4
    leaf = texts[chain[-1]]
    node = json.loads(leaf)["nodes"][0]
    assert node["name"] == "test" and node["size"] == 5 and len(node["content"]) == 1
    new = leaf.replace(b'"name":"test"', b'"name":"test.repaired"').replace(b'"size":5,', b"") \
        .replace(b'"content":["' + node["content"][0].encode() + b'"]', b'"content":[]')
    assert new.count(b"test.repaired") == 1 and b'"size"' not in new and b'"content":[]' in new
    want, saved = {}, []
    for old in reversed(chain):
        if old != chain[-1]:
            assert texts[old].count(prev_old.hex().encode()) == 1
            new = texts[old].replace(prev_old.hex().encode(), prev_new.hex().encode())
        prev_old, prev_new = old, hashlib.sha256(new).digest()
        want[old] = prev_new
        saved.append((prev_new, new))
    plan = r.plan()
    assert plan.changed == want and plan.unchanged == set()
    assert plan.new_trees == saved  # leaf first, as save_tree is reached
    assert plan.delete == [sid]
    (out,) = plan.snapshots
    assert (out.id, out.tree, out.new_tree) == (sid, chain[0], want[chain[0]])
    got = json.loads(out.text)
    assert got["original"] == sid.hex() and got["tags"] == ["repaired"] and got["id"] == sid.hex()
    assert got["tree"] == want[chain[0]].hex()
    assert {k: got[k] for k in snap if k not in ("tree", "tags")} == \
        {k: snap[k] for k in snap if k not in ("tree", "tags")}
    # the reference's listing of latest:home/thinkpad/data after repair
    (name, listed), = GOLDEN["nodes"].items()
    mine = json.loads(plan.new_trees[0][1])["nodes"]
    assert len(mine) == 1 and mine[0]["name"] == name == listed["name"]
    redacted = {k for k, v in listed.items() if isinstance(v, str) and v.startswith("[")}
    assert set(mine[0]) == set(listed) and "size" not in mine[0]
    assert {k: v for k, v in mine[0].items() if k not in redacted} == \
        {k: v for k, v in listed.items() if k not in redacted}
    assert mine[0]["content"] == [] and mine[0]["links"] == 1 and mine[0]["type"] == "file"


@pytest.mark.parametrize("name", [n for n in REPOS if n not in DAMAGED])
def test_plan_on_the_other_recorded_repositories(oracle_mod, name):
    """Every snapshot unchanged, nothing to save, nothing to delete -- but for
    repo-mixed: the index files every blob of a pack under the type of the
    pack's first blob (binarysorted.rs:127-163), its tree blobs lie in packs
    that begin with a data blob, so ``get_tree`` misses the snapshot's root as
    it does in the recorded ``check`` ("Tree ID ... not found in index"), and
    a root that cannot be loaded becomes the empty tree."""
    from rustic_core_amd.tree_write import EMPTY_TREE, EMPTY_TREE_ID
    r = recorded(name, oracle_mod)
    plan = r.plan()
    if name == "repo-mixed.tar.gz":
        (sid, _), = r.snapshots
        root = plan.snapshots[0].tree
        assert r.index.get_id(1, root) is None
        assert plan.changed == {root: EMPTY_TREE_ID} and plan.unchanged == set()
        assert plan.new_trees == [(EMPTY_TREE_ID, EMPTY_TREE)] and plan.delete == [sid]
        return
    assert plan.changed == {} and plan.new_trees == [] and plan.delete == []
    assert all(s.new_tree is None and s.text is None for s in plan.snapshots)
    assert len(plan.unchanged) == 4


def test_plan_on_repo_index_missing(oracle_mod):
    """Two snapshots, one tree the index lacks: it becomes the empty tree and
    its ancestors change."""
    from rustic_core_amd.tree_write import EMPTY_TREE, EMPTY_TREE_ID
    r = recorded("repo-index-missing.tar.gz", oracle_mod)
    assert len(r.snapshots) == 2
    plan = r.plan()
    roots = {s.id: s.tree for s in plan.snapshots}
    lost = [t for t in roots.values() if r.index.get_id(1, t) is None]
    assert len(lost) == 1
    assert plan.changed == {lost[0]: EMPTY_TREE_ID}
    assert plan.new_trees == [(EMPTY_TREE_ID, EMPTY_TREE)]
    assert plan.delete == [i for i, t in roots.items() if t == lost[0]]
    for s in plan.snapshots:
        assert (s.new_tree == EMPTY_TREE_ID) == (s.tree == lost[0])
    assert len(plan.unchanged) == 4


# ---- the serialiser, rule by rule ----------------------------------------------------------

def _round(text: bytes) -> bytes:
    from rustic_core_amd.tree_write import parse_tree_full, serialize_tree
    out, tid = serialize_tree(parse_tree_full(text))
    assert tid == hashlib.sha256(out).digest() and out.endswith(b"}\n")
    return out


def _tree(*nodes: str) -> bytes:
    return ('{"nodes":[' + ",".join(nodes) + "]}\n").encode()


@pytest.mark.parametrize("field", ("inode", "device_id", "size", "links"))
def test_a_u64_field_is_omitted_when_zero(field):
    keep = _tree('{"name":"f","type":"file","%s":3,"content":[]}' % field)
    assert _round(keep) == keep
    assert _round(keep.replace(b":3,", b":0,")) == _tree('{"name":"f","type":"file","content":[]}')


def test_none_is_skipped_in_metadata_and_content_null_is_written():
    src = _tree('{"name":"d","type":"dir","mode":null,"mtime":null,"uid":null,"user":null,'
                '"extended_attributes":[],"content":null,"subtree":null}')
    assert _round(src) == _tree('{"name":"d","type":"dir","content":null}')
    # absent content is null, an absent subtree stays absent, a present one is last
    assert _round(_tree('{"name":"d","type":"dir"}')) == _tree('{"name":"d","type":"dir","content":null}')
    sub = "ab" * 32
    with_sub = _tree('{"name":"d","type":"dir","content":null,"subtree":"%s"}' % sub)
    assert _round(with_sub) == with_sub


def test_symlink_with_and_without_linktarget_raw():
    a = _tree('{"name":"l","type":"symlink","linktarget":"../t","content":null}')
    b = _tree('{"name":"l","type":"symlink","linktarget":"t�","linktarget_raw":"dP8=","content":null}')
    assert _round(a) == a and _round(b) == b
    assert _round(a.replace(b'"content"', b'"linktarget_raw":null,"content"')) == a
    # linktarget on a node that is no symlink is no field of its type
    assert _round(_tree('{"name":"f","type":"file","linktarget":"","content":[]}')) == \
        _tree('{"name":"f","type":"file","content":[]}')


@pytest.mark.parametrize("tpe", ("dev", "chardev"))
def test_device_of_dev_and_chardev_is_always_written(tpe):
    a = _tree('{"name":"n","type":"%s","device":2049,"mode":8624,"content":null}' % tpe)
    assert _round(a) == a
    assert _round(_tree('{"name":"n","type":"%s","content":null}' % tpe)) == \
        _tree('{"name":"n","type":"%s","device":0,"content":null}' % tpe)


def test_extended_attributes_with_a_null_value():
    a = _tree('{"name":"f","type":"file","links":1,"extended_attributes":[{"name":"user.a","value":"YQ=="},'
              '{"name":"user.b","value":null}],"content":[]}')
    assert _round(a) == a
    assert _round(a.replace(b',"value":null', b"")) == a


def test_a_name_is_escaped_as_serde_json_escapes_it():
    a = _tree('{"name":"q\\"b\\\\c\\u0001\\n\\té€\U0001F600\x7f","type":"file","content":[]}')
    assert _round(a) == a
    # escapes that need none come back raw; \/ and upper-case hex are not kept
    assert _round(_tree('{"name":"\\u00e9\\/\\u001F","type":"file","content":[]}')) == \
        _tree('{"name":"é/\\u001f","type":"file","content":[]}')


def test_unknown_keys_are_dropped_and_keys_come_in_serdes_order():
    sub, c = "cd" * 32, "ef" * 32
    src = _tree('{"subtree":"%s","content":["%s"],"links":2,"size":9,"group":"g","user":"u","gid":2,"uid":1,'
                '"ctime":"%s","atime":"%s","mtime":"%s","mode":493,"generic_attributes":{"a":[1,{"b":2}]},'
                '"type":"file","inode":7,"device_id":8,"name":"n"}' % (sub, c, T, T, T))
    assert _round(src) == _tree(
        '{"name":"n","type":"file","mode":493,"mtime":"%s","atime":"%s","ctime":"%s","uid":1,"gid":2,'
        '"user":"u","group":"g","inode":7,"device_id":8,"size":9,"links":2,"content":["%s"],'
        '"subtree":"%s"}' % (T, T, T, c, sub))


def test_times_and_numbers_go_out_as_read_and_what_serde_refuses_raises():
    from rustic_core_amd.errors import RusticError
    from rustic_core_amd.tree_write import parse_tree_full
    odd = _tree('{"name":"f","type":"file","mtime":"2020-01-01T00:00:00Z","inode":18446744073709551615,'
                '"content":[]}')
    assert _round(odd) == odd
    for bad in ('{"name":"f","type":"file","size":1.0}', '{"name":"f","type":"file","size":-1}',
                '{"name":"f","type":"nope"}', '{"name":"f","type":"symlink"}', '{"type":"file"}',
                '{"name":"f","name":"g","type":"file"}', '{"name":"\\ud800","type":"file"}',
                '{"name":"f","type":"file","content":["abc"]}'):
        with pytest.raises(RusticError):
            parse_tree_full(_tree(bad))
    assert parse_tree_full(b'{"nodes":null}') == []


def test_a_snapshot_file_in_the_structs_order():
    from rustic_core_amd.tree_write import parse_snapshot, serialize_snapshot
    sid, tree = b"\x11" * 32, "22" * 32
    src = ('{"tags":["b","a","b"],"tree":"%s","time":"%s","paths":["/z","/a"],"uid":1e3,"gid":7,'
           '"hostname":"h","summary":{"files_new":3,"total_duration":1.50,"command":"x"},'
           '"unknown":1,"parent":null,"label":"","delete":"NotSet","description":null}' % (tree, T)).encode()
    got = serialize_snapshot(parse_snapshot(src), sid)
    assert got == ('{"time":"%s","tree":"%s","paths":["/a","/z"],"hostname":"h","username":"",'
                   '"uid":1e3,"gid":7,"tags":["a","b"],'
                   '"summary":{"files_new":3,"total_duration":1.50,"command":"x"},"id":"%s"}'
                   % (T, tree, sid.hex())).encode()
    assert b'"id"' not in serialize_snapshot(parse_snapshot(src), None)
    assert b'"id"' not in serialize_snapshot(parse_snapshot(src), bytes(32))
    full = ('{"time":"%s","program_version":"rustic 1","parent":"%s","parents":["%s"],"tree":"%s",'
            '"label":"L","paths":[],"hostname":"","username":"u","uid":0,"gid":0,"tags":[],'
            '"original":"%s","delete":"Never","description":"d","id":"%s"}'
            % (T, tree, tree, tree, tree, sid.hex())).encode()
    assert serialize_snapshot(parse_snapshot(full), sid) == full


# ---- the rules on built repositories --------------------------------------------------------

_BUILT = {}


def built(**kw) -> rr.HostRepo:
    key = tuple(sorted(kw.items()))
    if key not in _BUILT:
        repo = rr.build(no_content=kw.get("no_content", False))
        names = {v: k for k, v in repo.names.items()}
        _BUILT[key] = rr.HostRepo(repo, without=[names[n] for n in kw.get("without", ())])
    return _BUILT[key]


def _expected(h: rr.HostRepo):
    """{tree name: new text} of the trees that change in repair_repo.build()
    with ``lostleaf`` out of the index, built here as objects."""
    f, d, ln = rr.f, rr.d, h.length
    new = {}
    new["nosub"] = [d("hollow", rr.EMPTY_ID), f("ok", ["a.0"], ln("a.0"), n=1)]  # its size too
    new["zero"] = [f("z.repaired", ["a.1"], ln("a.1"), n=2)]
    new["twin1"] = new["twin2"] = [f("x.repaired", ["a.3"], ln("a.3"), n=5)]
    new["already"] = [f("y.repaired", [], n=6)]
    new["sizefix"] = [f("wrong", ["a.4", "a.5"], ln("a.4") + ln("a.5"), n=7),
                      f("cut.repaired", ["a.6"], ln("a.6"), n=8)]
    new["lostleaf"] = []
    text = {k: rr.tree_text(v) for k, v in new.items()}
    nid = {k: rr.tid(v) for k, v in text.items()}
    text["keeps"] = rr.tree_text([d("gone", nid["lostleaf"]), f("stays", ["a.8"], ln("a.8"), n=10)])
    nid["keeps"] = rr.tid(text["keeps"])
    same = {"fifo", "nondir", "sameid", "sizeonly"}
    text["rules"] = rr.tree_text([d(k, h.names[k] if k in same else nid[k]) for k in
                                  ("nosub", "zero", "fifo", "sameid", "twin1", "twin2",
                                   "already", "sizefix", "sizeonly", "keeps")])
    text["backleaf"] = rr.tree_text([f("b.repaired", ["a.9"], ln("a.9"), n=11)])
    text["P"] = rr.tree_text([d("leafd", rr.tid(text["backleaf"]))])
    text["R"] = rr.tree_text([d("back", rr.tid(text["P"]))])
    text["Q"] = rr.tree_text([d("r", rr.tid(text["R"]))])
    text["backroot"] = rr.tree_text([d("p", rr.tid(text["P"])), d("q", rr.tid(text["Q"]))])
    # the tree with the unknown key: rewritten without it
    text["hostbelow"] = rr.tree_text([f("hb.repaired", ["a.11"], ln("a.11"), n=14)])
    text["host"] = rr.tree_text([f("hf.repaired", ["a.10"], ln("a.10"), n=15),
                                 d("below", rr.tid(text["hostbelow"]))])
    text["hostroot"] = rr.tree_text([d("host", rr.tid(text["host"]))])
    return text


def test_every_rule_on_the_built_repository():
    h = built(without=("lostleaf",))
    want = _expected(h)
    plan = h.plan()
    name = lambda t: h.repo.names.get(t, t.hex())
    assert {name(k): v for k, v in plan.changed.items()} == {k: rr.tid(v) for k, v in want.items()}
    # a dir without a subtree, an all-zero id, the size corrected beside a cut file: in ``want``.
    # kept as they are: the fifo with a missing id, the tree under a symlink (never visited: in
    # neither set), the tree whose new id is its old one, the size that alone is wrong
    assert {name(t) for t in plan.unchanged} == \
        {"fifo", "nondir", "oddroot", "sameid", "sizeonly", "cleanroot", rr.EMPTY_ID.hex()}
    assert h.names["hidden"] not in plan.unchanged and h.names["hidden"] not in plan.changed
    # saved: each id once (the twins' tree, the empty tree of ``hollow``, ``void`` and
    # ``lostleaf``), not the tree the index has; children before parents
    saved = [i for i, _ in plan.new_trees]
    assert len(set(saved)) == len(saved)
    assert dict(plan.new_trees) == {rr.tid(v): v for k, v in want.items() if k != "already"} | \
        {rr.EMPTY_ID: rr.EMPTY}
    assert rr.tid(want["already"]) == h.names["already-repaired"]
    at = {i: n for n, i in enumerate(saved)}
    assert at[rr.EMPTY_ID] == 0  # ``hollow`` is the first thing the walk saves
    for parent, child in (("rules", "nosub"), ("rules", "keeps"), ("P", "backleaf"), ("R", "P"),
                          ("Q", "R"), ("backroot", "Q"), ("backroot", "P")):
        assert at[rr.tid(want[child])] < at[rr.tid(want[parent])]
    # snapshots: two changed, the clean one not
    s0, s1, s2, s3, s4 = plan.snapshots
    assert (s0.new_tree, s1.new_tree, s2.new_tree, s3.new_tree, s4.new_tree) == \
        (rr.tid(want["rules"]), rr.tid(want["backroot"]), None, None, rr.tid(want["hostroot"]))
    assert plan.delete == [s0.id, s1.id, s4.id] and s2.text is None and s3.text is None
    assert b"generic_attributes" in h.repo.trees[h.names["host"]]
    assert b"generic_attributes" not in want["host"]
    got = json.loads(s0.text)
    assert got["tags"] == ["repaired"] and got["original"] == s0.id.hex() and got["hostname"] == "host0"


def test_options_suffix_tags_delete_and_original_kept():
    from rustic_core_amd.repair import RepairSnapshotsOptions
    h = built(without=("lostleaf",))
    sealed = rr.snapshot_file(h.repo.snapshots[1], 1, original="77" * 32, tags=["x"])
    sid = hashlib.sha256(sealed).digest()
    plan = h.plan(RepairSnapshotsOptions(delete=False, suffix="~", tags=("b,a", "c")), [(sid, sealed)])
    assert plan.delete == []
    got = json.loads(plan.snapshots[0].text)
    assert got["tags"] == ["a", "b", "c"] and got["original"] == "77" * 32
    assert b'"b~"' in dict(plan.new_trees)[plan.changed[h.names["backleaf"]]]


def test_a_file_without_content_raises_with_its_path():
    from rustic_core_amd.errors import ErrorKind, RusticError
    h = built(no_content=True)
    with pytest.raises(RusticError) as e:
        h.plan()
    assert e.value.kind == ErrorKind.Internal and '`a/b"q/nc`' in str(e.value)
    h.plan(snapshots=h.snapshots[:5])  # the other snapshots alone: fine


def test_append_only_with_delete_is_refused_before_any_work():
    from rustic_core_amd.chunker import ConfigFile
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.repair import RepairSnapshotsOptions, plan_repair, repair_snapshots

    def never(*a):
        raise AssertionError("work was done")
    cfg = ConfigFile(append_only=True)
    for call in (lambda o: plan_repair(None, None, [(b"", b"")], never, o, device=None, config=cfg),
                 lambda o: repair_snapshots(None, None, [(b"", b"")], never, cfg, o, device=None)):
        with pytest.raises(RusticError) as e:
            call(RepairSnapshotsOptions())
        assert e.value.kind == ErrorKind.AppendOnly
    h = built(without=("lostleaf",))
    plan = plan_repair(h.key, h.index, h.snapshots, h.read_partial,
                       RepairSnapshotsOptions(delete=False), device=None, config=cfg)
    assert plan.delete == [] and len(plan.changed) > 5


# ---- the models against the rule --------------------------------------------------------------

def _model_verdict(h: rr.HostRepo, snapshots):
    """The device's verdict by the models, every tree of the walk in one
    batch: ({tree id: damaged}, {tree id: changed}, counts, rounds are not
    modelled)."""
    repo = h.repo
    walked, frontier = [], list(dict.fromkeys(snapshots))
    seen = set(frontier)
    while frontier:  # the walk: only subtrees of dir nodes, lost trees are not read
        walked += frontier
        nxt = []
        for t in frontier:
            if t not in h.index:
                continue
            for n in json.loads(repo.trees[t])["nodes"]:
                s = n.get("subtree")
                if n["type"] == "dir" and s and bytes.fromhex(s) not in seen:
                    seen.add(bytes.fromhex(s))
                    nxt.append(bytes.fromhex(s))
        frontier = nxt
    slot = {t: i for i, t in enumerate(walked)}
    read = [t for t in walked if t in h.index]
    rec = tnm.records([repo.trees[t] for t in read])
    assert not any(rec.status)
    data_hits = [(1, 0) if i in h.index else (0, 0) for i in rec.data_ids]
    tree_hits = [(1, slot[i]) if i in slot else (0, 0xFFFFFFFF) for i in rec.tree_ids]
    damaged, edges, counts = model.level_model(tnm.node_array(rec.nodes), data_hits, tree_hits,
                                               rec.is_dir, [slot[t] for t in read], len(walked))
    flags = np.zeros(len(walked), np.uint8)
    flags[damaged] = 1
    flags[[slot[t] for t in walked if t not in h.index]] = 1  # lost: the walk's own flag
    changed = model.spread_model(edges, flags)
    return walked, flags, changed, edges, counts


def test_models_against_the_python_rule():
    h = built(without=("lostleaf",))
    # all but the snapshot of the tree outside the device's grammar, which gives no records
    walked, damaged, changed, edges, counts = _model_verdict(h, h.repo.snapshots[:4])
    plan = h.plan(snapshots=h.snapshots[:4])
    name = lambda t: h.repo.names.get(t, "empty")
    assert {name(t) for t, f in zip(walked, damaged) if f} == \
        {"nosub", "zero", "twin1", "twin2", "already", "sizefix", "lostleaf", "backleaf", "empty"}
    # changed by the spread: what the rule changes, and the tree whose new id is its old one
    # (the empty tree, lost) with the tree above it, which the id compare then takes back
    assert {t for t, f in zip(walked, changed) if f} == set(plan.changed) | {rr.EMPTY_ID, h.names["sameid"]}
    assert set(walked) == set(plan.changed) | plan.unchanged
    # zero, twin1, twin2, already, sizefix/cut, backleaf: six files with one missing id each
    # (the fifo's is not looked at, ``hidden`` is never read); with ``hollow`` seven nodes
    assert counts == (6, 7, 0, model.NO_NODE)
    # the subtree of the symlink has no edge; every dir subtree has one
    assert (edges == model.NO_EDGE).all(axis=1).sum() == 1
    # a single bottom-up sweep over the levels misses R and Q: the fixed point does not
    assert {h.names[n] for n in ("P", "R", "Q", "backroot")} <= set(plan.changed)


def test_model_counts_and_no_content():
    h = built(no_content=True)
    _, _, _, _, counts = _model_verdict(h, h.repo.snapshots[:4] + h.repo.snapshots[5:])
    assert counts[2] == 1 and counts[3] != model.NO_NODE


def test_spread_model_on_hand_made_graphs():
    no = model.NO_EDGE
    chain = [(i, i + 1) for i in range(9)]
    assert model.spread_model(chain, [0] * 9 + [1]).tolist() == [1] * 10
    assert model.spread_model(chain, [0] * 5 + [1] + [0] * 4).tolist() == [1] * 6 + [0] * 4
    diamond = [(0, 1), (0, 2), (1, 3), (2, 3), (4, 0)]
    assert model.spread_model(diamond, [0, 0, 0, 1, 0, 0]).tolist() == [1, 1, 1, 1, 1, 0]
    cycle = [(0, 1), (1, 2), (2, 0), (3, 0), (1, 4)]
    assert model.spread_model(cycle, [0, 0, 1, 0, 0]).tolist() == [1, 1, 1, 1, 0]
    assert model.spread_model([(no, no), (0, no), (no, 1)], [0, 1]).tolist() == [0, 1]
    assert model.spread_model(np.zeros((0, 2)), [1, 0]).tolist() == [1, 0]


def test_level_model_ties_in_data_start():
    """Files with no ids between files with ids share a data_start with their
    neighbour: the id's node is the last record that starts at or before it."""
    nodes = tnm.node_array([
        (0, 0, 0, 0, 0, 0, 0, 1, 0),  # file, content []
        (0, 0, 0, 0, 2, 0, 0, 1, 0),  # file, ids 0, 1
        (0, 0, 0, 2, 5, 0, 5, 1, 0),  # a fifo with 5 ids: none of them in d_data_ids
        (0, 0, 1, 2, 0, 0, 0, 1, 0),  # file, content [] (blob 1)
        (0, 0, 1, 2, 1, 0, 0, 1, 0),  # file, id 2
        (0, 0, 2, 3, 0, 0, 0, 0, 0),  # file without content (blob 2)
        (0, 0, 2, 3, 0, 0, 1, 0, 0),  # dir without subtree
    ])
    hits = lambda miss: [(0, 0) if i in miss else (1, 3) for i in range(3)]
    lv = lambda miss: model.level_model(nodes, hits(miss), [], [], [10, 11, 12], 20)
    assert lv(())[0] == [12] and lv(())[2] == (0, 1, 1, 5)
    assert lv((0,))[0] == [10, 12] and lv((1,))[0] == [10, 12]
    assert lv((2,))[0] == [11, 12] and lv((2,))[2] == (1, 2, 1, 5)
    assert lv((0, 1, 2))[2] == (3, 3, 1, 5)


# ---- the ABI without a device ------------------------------------------------------------------

def test_symbols_and_abi_version(rcdc_lib):
    from rustic_core_amd import _lib
    assert all(s in _lib.EXPORTS and hasattr(rcdc_lib, s) for s in SYMBOLS)
    assert rcdc_lib.rcdc_abi_version() == 5
    assert rcdc_lib.rcdc_repair_spread_rounds_per_launch() >= 1


def test_repair_trees_level_refused_before_any_hip_call(rcdc_lib):
    from rustic_core_amd import _lib
    L = rcdc_lib
    fake, res = ctypes.c_void_p(64), _lib.RepairLevelResult(1, 2, 3, 4)
    base = dict(ctx=fake, nodes=fake, n_nodes=3, data_hits=fake, n_data=4, is_dir=fake, tree_hits=fake,
                n_tree=2, slot=fake, n_blobs=2, damaged=fake, n_slots=9, edges=fake,
                res=ctypes.byref(res))

    def call(**kw):
        a = dict(base, **kw)
        return L.rcdc_repair_trees_level(
            a["ctx"], a["nodes"], a["n_nodes"], a["data_hits"], a["n_data"], a["is_dir"],
            a["tree_hits"], a["n_tree"], a["slot"], a["n_blobs"], a["damaged"], a["n_slots"],
            a["edges"], a["res"], None)
    assert call(ctx=None) == 2 and "ctx is NULL" in _lib.last_error()
    assert call(res=ctypes.POINTER(_lib.RepairLevelResult)()) == 2 and "result is NULL" in _lib.last_error()
    for k in ("nodes", "data_hits", "is_dir", "tree_hits", "slot", "damaged", "edges"):
        assert call(**{k: None}) == 2 and "null array" in _lib.last_error(), k
    assert call(nodes=ctypes.c_void_p(72)) == 2 and "16-byte" in _lib.last_error()
    assert call(edges=ctypes.c_void_p(68)) == 2 and "8-byte" in _lib.last_error()
    for k in ("data_hits", "tree_hits", "slot"):
        assert call(**{k: ctypes.c_void_p(66)}) == 2 and "4-byte" in _lib.last_error(), k
    for k in ("n_nodes", "n_data", "n_tree", "n_blobs", "n_slots"):
        assert call(**{k: 2 ** 32 - 1}) == 2 and "2^32" in _lib.last_error(), k
    # no nodes: nothing is launched
    assert call(n_nodes=0, nodes=None) == 0
    assert (res.missing_ids, res.damaged_nodes, res.files_without_content) == (0, 0, 0)
    assert res.first_without_content == 2 ** 64 - 1


def test_repair_spread_refused_before_any_hip_call(rcdc_lib):
    from rustic_core_amd import _lib
    L = rcdc_lib
    fake, rounds = ctypes.c_void_p(64), ctypes.c_uint64(5)

    def call(ctx=fake, edges=fake, n=3, damaged=fake, changed=fake, k=4, rounds_=None):
        return L.rcdc_repair_spread(ctx, edges, n, damaged, changed, k,
                                    ctypes.byref(rounds) if rounds_ is None else rounds_, None)
    assert call(ctx=None) == 2 and "ctx is NULL" in _lib.last_error()
    assert call(rounds_=ctypes.POINTER(ctypes.c_uint64)()) == 2 and "rounds is NULL" in _lib.last_error()
    for kw in ({"edges": None}, {"damaged": None}, {"changed": None}):
        assert call(**kw) == 2 and "null array" in _lib.last_error(), kw
    assert call(edges=ctypes.c_void_p(68)) == 2 and "8-byte" in _lib.last_error()
    assert call(n=2 ** 32 - 1) == 2 and call(k=2 ** 32 - 1) == 2 and "2^32" in _lib.last_error()
    # no slots: nothing is launched
    assert call(k=0, damaged=None, changed=None) == 0 and rounds.value == 0
