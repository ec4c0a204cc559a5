"""CPU: the node records of rcdc_tree_nodes -- the model of G_N and of the
records (tests/tree_nodes_model.py) against ``tree.parse_tree_nodes_host``,
check_trees' level rule against hand-written expectations, and the argument
checks of rcdc_tree_nodes, rcdc_tree_names and rcdc_check_trees_level without
a device."""
import ctypes
import json

import numpy as np
import pytest

from tests import tree_json_model as gt
from tests import tree_nodes_model as model
from tests.check_cases import REPOS, Repo
from tests.index_json_cases import hid
from tests.test_used_blobs_host import OracleKey

SYMBOLS = ("rcdc_tree_nodes", "rcdc_tree_nodes_bound", "rcdc_tree_names", "rcdc_check_trees_level")


@pytest.mark.parametrize("name,data,in_gt,in_gn", model.TABLE, ids=[c[0] for c in model.TABLE])
def test_model_judges_the_table(name, data, in_gt, in_gn):
    assert gt.in_gt(data) == in_gt and model.in_gn(data) == in_gn
    assert in_gn or not in_gt  # G_N is G_T with one rule dropped: nothing leaves


def test_table_has_the_new_cases():
    by_name = {c[0]: c for c in model.TABLE}
    for dropped in ("dir_without_subtree", "dir_subtree_null", "gn_dir_without_subtree",
                    "gn_dir_subtree_null"):
        assert by_name[dropped][2:] == (False, True)
    # the three kinds of content and the names the issue lists
    facts = lambda n: model.node_facts(by_name[n][1])
    assert facts("gn_file_without_content")[0][1] is None
    assert facts("gn_file_content_null")[0][1] is None
    assert facts("gn_file_content_empty")[0][1] == []
    raw = lambda n: [by_name[n][1][a:a + ln] for a, ln, _ in model.name_spans(by_name[n][1])]
    assert raw("gn_name_empty") == [b""] and raw("gn_name_escaped_quote") == [b'a\\"b']
    assert raw("gn_name_unicode_escape") == [b"\\u00e9"]
    assert raw("gn_name_raw_utf8") == ["é€\U0001F600".encode()]
    assert raw("gn_name_leading_slash") == [b"/abs/path"]
    assert raw("gn_xattr_named_name") == [b"real"] and raw("gn_user_named_name") == [b"f"]
    assert [e for _, _, e in model.name_spans(by_name["gn_name_escaped_quote"][1])] == [True]
    assert [e for _, _, e in model.name_spans(by_name["gn_name_raw_utf8"][1])] == [False]


def test_parse_tree_nodes_host_against_the_model():
    """Facts and names: the span's raw bytes between quotes are the name
    ``json.loads`` gives."""
    from rustic_core_amd.check import raw_name
    from rustic_core_amd.tree import NODE_TYPES, parse_tree_nodes_host
    assert NODE_TYPES == model.TYPES
    n_nodes = 0
    for name, data, _, in_gn in model.TABLE:
        if not in_gn:
            continue
        host = parse_tree_nodes_host(data)
        facts, spans = model.node_facts(data), model.name_spans(data)
        assert len(host) == len(facts) == len(spans), name
        for h, (tpe, content, subtree), (at, ln, esc) in zip(host, facts, spans):
            assert (NODE_TYPES.index(h.type), h.content, h.subtree) == (tpe, content, subtree), name
            assert raw_name(data[at:at + ln]) == h.name, name
            assert esc == (b"\\" in data[at:at + ln])
            n_nodes += 1
    assert n_nodes > 80


def test_records_of_a_batch():
    """The running counts over a batch with a blob outside G_N in it."""
    by_name = {c[0]: c[1] for c in model.TABLE}
    blobs = [by_name["gn_dir_without_subtree_between"], by_name["unknown_key"],
             by_name["gn_three_contents"], by_name["non_file_with_content"]]
    m = model.records(blobs, [0, 1000, 2000, 3000])
    assert m.status == [0, 1, 0, 0]
    assert m.blobs == [(4, 3, 1, 0, 0, 0), (0, 0, 0, 3, 1, 4), (5, 2, 0, 3, 1, 4), (3, 1, 1, 5, 1, 9)]
    rec = model.node_array(m.nodes)
    assert rec["blob"].tolist() == [0] * 4 + [2] * 5 + [3] * 3
    assert rec["data_start"].tolist() == [0, 2, 2, 2, 3, 3, 3, 3, 5, 5, 5, 5]
    assert rec["n_content"].tolist() == [2, 0, 0, 1, 0, 0, 0, 2, 0, 2, 1, 1]
    assert (rec["flags"] & model.CONTENT).tolist() == [1, 0, 0, 1, 0, 0, 1, 1, 1, 1, 1, 1]
    assert rec["tree_index"].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 2, 2]
    assert rec["type"].tolist() == [0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 6, 0]
    assert rec["name_off"][4] == 2000 + blobs[2].index(b'"f"') + 1 and rec["name_len"][4] == 1


# ---- the level rule ---------------------------------------------------------------------

def _node(name, tpe, content=None, subtree=None):
    from rustic_core_amd.tree import TreeNode
    return TreeNode(name, tpe, content, subtree)


def test_level_rule_each_kind_and_the_order():
    from rustic_core_amd.check import ERROR, Finding, judge_level, level_ids
    ok, gone, null = bytes([1]) * 32, bytes([2]) * 32, bytes(32)
    sub, sub_gone = bytes([3]) * 32, bytes([4]) * 32
    level = [("", [_node("none", "file"), _node("empty", "file", []),
                   _node("four", "file", [ok, null, gone, null]),
                   _node("nosub", "dir"), _node("nullsub", "dir", None, null),
                   _node("lost", "dir", None, sub_gone), _node("fine", "dir", None, sub),
                   _node("link", "symlink", [gone], sub)]),
             ("/abs", [_node("/top", "file"), _node("rel", "dir")])]
    data_ids, tree_ids = level_ids(level)
    assert data_ids == [ok, null, gone, null] and tree_ids == [sub_gone, sub]
    pack = {ok: b"P1", sub: b"P2"}
    findings, packs = [], set()
    below = judge_level(level, [pack.get(i) for i in data_ids], [pack.get(i) for i in tree_ids],
                        findings, packs)
    f = lambda kind, **kw: (ERROR, Finding(kind, kw))
    assert findings == [
        f("FileHasNoContent", file="none"),
        f("FileBlobHasNullId", file="four", blob_num=1),
        f("FileBlobNotInIndex", file="four", blob_id=null),
        f("FileBlobNotInIndex", file="four", blob_id=gone),
        f("FileBlobHasNullId", file="four", blob_num=3),
        f("FileBlobNotInIndex", file="four", blob_id=null),
        f("NoSubTree", dir="nosub"),
        f("NullSubTree", dir="nullsub"),
        f("SubTreeMissingInIndex", dir="lost", blob_id=sub_gone),
        f("FileHasNoContent", file="/top"),
        f("NoSubTree", dir="/abs/rel"),
    ]
    assert packs == {b"P1", b"P2"}
    assert below == [(null, "nullsub"), (sub_gone, "lost"), (sub, "fine"), (sub, "link")]


def test_level_rule_of_the_model_agrees():
    """The rule over node records (the model rcdc_check_trees_level is held
    against) gives what ``judge_level`` gives for the same nodes."""
    from rustic_core_amd.check import judge_level, level_ids
    from rustic_core_amd.tree import parse_tree_nodes_host
    ok, null = bytes.fromhex(hid(1)), bytes(32)
    text = json.dumps({"nodes": [
        {"name": "a", "type": "file"}, {"name": "b", "type": "file", "content": []},
        {"name": "c", "type": "file", "content": [hid(1), null.hex(), hid(2), null.hex()]},
        {"name": "d", "type": "dir"}, {"name": "e", "type": "dir", "subtree": null.hex()},
        {"name": "f", "type": "dir", "subtree": hid(3)}, {"name": "g", "type": "dir", "subtree": hid(4)},
        {"name": "h", "type": "fifo", "content": [hid(2)], "subtree": hid(5)}]}).encode()
    m = model.records([text])
    hits_of = lambda ids, have: [(1, have[i]) if i in have else (0, 0) for i in ids]
    found, dp, tp = model.level_rule(m.nodes, m.data_ids, hits_of(m.data_ids, {ok: 7}),
                                     m.tree_ids, hits_of(m.tree_ids, {bytes.fromhex(hid(4)): 9}))
    level = [("", parse_tree_nodes_host(text))]
    data_ids, tree_ids = level_ids(level)
    findings, packs = [], set()
    judge_level(level, ["P7" if i == ok else None for i in data_ids],
                ["P9" if i == bytes.fromhex(hid(4)) else None for i in tree_ids], findings, packs)
    names = "abcdefgh"
    assert [(names[k], model.KINDS[kind]) for k, kind, _ in found] == \
        [(dict(x.fields).get("file", dict(x.fields).get("dir")), x.kind) for _, x in findings]
    assert [n for _, kind, n in found if kind == 1] == [1, 3]
    assert (dp, tp, packs) == ({7}, {9}, {"P7", "P9"})


@pytest.mark.parametrize("seed", range(6))
def test_level_rule_in_numpy_agrees(seed):
    """``level_rule_np`` (the reference of the level of 2^20 nodes in
    tests/test_gpu_check_trees.py) against ``level_rule`` on random levels:
    every type, nodes with and without content and subtree, null ids, ids the
    index lacks, both, and hits whose pack is NO_PACK."""
    rng = np.random.default_rng(seed)
    null = bytes(32)
    nodes, data_ids, data_hits, tree_ids, tree_hits = [], [], [], [], []

    def an_id():
        return null if rng.random() < 0.2 else bytes(rng.integers(1, 256, 32, dtype=np.uint8))

    def a_hit():
        r = rng.random()
        return (0, 0) if r < 0.2 else (1, model.NO_PACK) if r < 0.3 else (1, int(rng.integers(0, 30)))
    for _ in range(int(rng.integers(1, 120))):
        tpe = int(rng.choice([0, 0, 0, 1, 1, 2, 5]))
        content = rng.random() < 0.8
        nc = int(rng.integers(0, 6)) if content else 0
        sub = rng.random() < (0.8 if tpe == 1 else 0.2)
        nodes.append((0, 0, 0, len(data_ids), nc, len(tree_ids), tpe,
                      (model.CONTENT if content else 0) | (model.SUBTREE if sub else 0), 0))
        if tpe == 0:
            for _ in range(nc):
                data_ids.append(an_id())
                data_hits.append(a_hit())
        if sub:
            tree_ids.append(an_id())
            tree_hits.append(a_hit())
    want = model.level_rule(nodes, data_ids, data_hits, tree_ids, tree_hits)
    arr = lambda ids: np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32)
    found, dp, tp = model.level_rule_np(model.node_array(nodes), arr(data_ids), data_hits,
                                        arr(tree_ids), tree_hits)
    assert [tuple(r) for r in found.tolist()] == want[0] and (dp, tp) == want[1:]
    assert seed or len({k for _, k, _ in want[0]}) == 6  # every kind


# ---- the recorded repositories ----------------------------------------------------------

def test_tree_blobs_of_the_recorded_repositories_outside_gn(oracle_mod, monkeypatch, capsys):
    """How many tree blobs of each recorded repository the device route of
    check_trees hands to the host: counted here with the model, asserted on
    the device in tests/test_gpu_check_trees.py."""
    from oracle import zstd_ref as zr
    from rustic_core_amd import tree
    from rustic_core_amd.check import check_repository
    counted = {}
    for name in REPOS:
        texts = []
        inner = tree.parse_tree_nodes_host
        monkeypatch.setattr(tree, "parse_tree_nodes_host",
                            lambda text, inner=inner: (texts.append(bytes(text)), inner(text))[1])
        repo = Repo(name, oracle_mod)
        k = OracleKey(oracle_mod, repo.master)
        trees = tree.snapshot_trees(k, repo.snapshots(), device=None, decode=zr.decompress)
        check_repository(k, repo.list_with_size, repo.read_full, repo.read_partial, trees,
                         device=None, decode=zr.decompress)
        monkeypatch.setattr(tree, "parse_tree_nodes_host", inner)
        counted[name] = sum(not model.in_gn(t) for t in texts)
        with capsys.disabled():
            print(f"\n{name}: {len(texts)} tree blobs, {counted[name]} outside G_N")
    assert counted == model.OUTSIDE_GN


# ---- the ABI without a device ---------------------------------------------------------

def test_symbols_and_structs(rcdc_lib):
    from rustic_core_amd import _lib
    from rustic_core_amd.check import CKT_FINDING
    from rustic_core_amd.tree import TR_BLOB, TR_NODE, TR_NODES_BLOB, parse_bound
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    assert TR_NODE.itemsize == 32 and TR_NODES_BLOB.itemsize == 40 and CKT_FINDING.itemsize == 16
    assert TR_NODES_BLOB.names[:-1] == TR_BLOB.names and TR_BLOB.itemsize == 32
    assert TR_NODE.fields["type"][1] == 28 and TR_NODE.fields["flags"][1] == 29
    # the bound is rcdc_tree_parse_bound's: the smallest node of G_N has 24 bytes too
    small = b'{"name":"","type":"dir"}'
    assert len(small) == 24 and model.in_gn(b'{"nodes":[' + small + b"]}")
    d, t, n = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    for length in (0, 23, 24, 25, 49, 1000, 4097):
        rcdc_lib.rcdc_tree_nodes_bound(length, ctypes.byref(d), ctypes.byref(t), ctypes.byref(n))
        assert (d.value, t.value, n.value) == parse_bound(length)
    for k in (1, 2, 50):
        assert parse_bound(len(b",".join([small] * k)))[2] == k


def test_tree_nodes_refused_before_any_hip_call(rcdc_lib):
    from rustic_core_amd import _lib
    from rustic_core_amd.tree import TR_NODES_BLOB
    L = rcdc_lib
    res = _lib.TrparseResult()
    n_text = 67 * 4  # bound: 4 content ids, 2 subtrees, 10 nodes
    refs = (_lib.IxparseRef * 1)(_lib.IxparseRef(0, n_text))
    blobs = np.zeros(1, TR_NODES_BLOB)
    fake = ctypes.c_void_p(64)  # stands for device memory / a context; never read
    r, b, rs = ctypes.addressof(refs), blobs.ctypes.data, ctypes.byref(res)

    def call(ctx=fake, text=fake, text_len=n_text, refs_=r, n=1, data=fake, cap_d=4, tree=fake,
             is_dir=fake, cap_t=2, nodes=fake, cap_n=10, blobs_=b, res_=rs):
        return L.rcdc_tree_nodes(ctx, text, text_len, refs_, n, data, cap_d, tree, is_dir, cap_t,
                                 nodes, cap_n, blobs_, res_, None)
    assert call(ctx=None) == 2 and "rcdc_tree_nodes: ctx is NULL" in _lib.last_error()
    assert call(res_=None) == 2
    for kw in ({"refs_": None}, {"blobs_": None}, {"text": None}):
        assert call(**kw) == 2, kw
    assert call(text_len=n_text - 1) == 2 and "outside the arena" in _lib.last_error()
    assert call(cap_d=3) == 2 and "below" in _lib.last_error()
    assert call(cap_t=1) == 2 and "below" in _lib.last_error()
    assert call(data=ctypes.c_void_p(72)) == 2 and "aligned" in _lib.last_error()
    # the three refusals of its own
    assert call(nodes=None) == 2 and "d_nodes is NULL" in _lib.last_error()
    assert call(cap_n=9) == 2 and "below" in _lib.last_error()
    assert call(nodes=ctypes.c_void_p(72)) == 2 and "d_nodes must be 16-byte aligned" in _lib.last_error()
    # n == 0 launches nothing
    res.nodes = 7
    assert L.rcdc_tree_nodes(fake, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, rs,
                             None) == 0
    assert res.nodes == 0


def test_tree_names_refused_before_any_hip_call(rcdc_lib):
    from rustic_core_amd import _lib
    L = rcdc_lib
    fake, total = ctypes.c_void_p(64), ctypes.c_uint64(5)

    def call(ctx=fake, text=fake, nodes=fake, index=fake, n=3, offsets=fake, names=fake, total_=None):
        return L.rcdc_tree_names(ctx, text, 100, nodes, 4, index, n, offsets, names, 10,
                                 ctypes.byref(total) if total_ is None else total_, None)
    assert call(ctx=None) == 2 and "ctx is NULL" in _lib.last_error()
    assert call(total_=ctypes.POINTER(ctypes.c_uint64)()) == 2 and "total is NULL" in _lib.last_error()
    for kw in ({"index": None}, {"offsets": None}, {"nodes": None}, {"text": None}):
        assert call(**kw) == 2 and "NULL" in _lib.last_error().upper(), kw
    for kw in ({"index": ctypes.c_void_p(66)}, {"offsets": ctypes.c_void_p(68)},
               {"nodes": ctypes.c_void_p(72)}):
        assert call(**kw) == 2 and "misaligned" in _lib.last_error(), kw
    assert call(n=2 ** 32 - 1) == 2
    # an empty list launches nothing
    assert call(n=0, index=None, offsets=None, names=None) == 0 and total.value == 0


def test_check_trees_level_refused_before_any_hip_call(rcdc_lib):
    from rustic_core_amd import _lib
    L = rcdc_lib
    fake, count = ctypes.c_void_p(64), ctypes.c_uint64(5)
    base = dict(ctx=fake, nodes=fake, n_nodes=3, data=fake, data_hits=fake, n_data=4, tree=fake,
                is_dir=fake, tree_hits=fake, n_tree=2, dmarks=fake, n_dp=5, tmarks=fake, n_tp=6,
                findings=fake, cap=8, count=ctypes.byref(count))

    def call(**kw):
        a = dict(base, **kw)
        return L.rcdc_check_trees_level(
            a["ctx"], a["nodes"], a["n_nodes"], a["data"], a["data_hits"], a["n_data"], a["tree"],
            a["is_dir"], a["tree_hits"], a["n_tree"], a["dmarks"], a["n_dp"], a["tmarks"], a["n_tp"],
            a["findings"], a["cap"], a["count"], None)
    assert call(ctx=None) == 2 and "ctx is NULL" in _lib.last_error()
    assert call(count=ctypes.POINTER(ctypes.c_uint64)()) == 2
    for k in ("nodes", "data", "data_hits", "tree", "is_dir", "tree_hits", "dmarks", "tmarks"):
        assert call(**{k: None}) == 2 and "null array" in _lib.last_error(), k
    assert call(findings=None) == 2 and "d_findings is NULL" in _lib.last_error()
    for k in ("nodes", "data", "tree", "findings"):
        assert call(**{k: ctypes.c_void_p(72)}) == 2 and "16-byte" in _lib.last_error(), k
    for k in ("data_hits", "tree_hits"):
        assert call(**{k: ctypes.c_void_p(66)}) == 2 and "4-byte" in _lib.last_error(), k
    for k in ("n_nodes", "n_data", "n_tree"):
        assert call(**{k: 2 ** 32 - 1}) == 2 and "2^32" in _lib.last_error(), k
    # no nodes: nothing is launched and nothing is found
    assert call(n_nodes=0, nodes=None) == 0 and count.value == 0
    assert call(n_nodes=0, nodes=None, findings=None, cap=0, n_data=0, data=None, data_hits=None,
                n_tree=0, tree=None, is_dir=None, tree_hits=None, n_dp=0, dmarks=None, n_tp=0,
                tmarks=None) == 0
