"""Node records on the device (rcdc_tree_nodes, tree.parse_tree_nodes) and raw
names gathered (rcdc_tree_names, tree.tree_names) against the plain-Python
model of tests/tree_nodes_model.py."""
import random

import numpy as np
import pytest

from tests import tree_json_model as gt
from tests import tree_nodes_model as model
from tests.index_json_cases import hid
from tests.test_gpu_tree_parse import _arena, _arena_layout, _long_blobs, _many_tile_blobs, _tiles
from tests.tree_json_cases import (CASES, dir_node, file_node, flipped, other_node, random_text,
                                   random_tree, serialize, tree)

pytestmark = pytest.mark.gpu

GUARD = 256


def _check(blobs, align=1, shift=0):
    """``blobs`` through rcdc_tree_nodes in one call: statuses, per-blob
    records, id arrays and node records equal the model's, and nothing is
    written past the counts reported (0xA5 fill and guard)."""
    from rustic_core_amd.tree import parse_tree_nodes
    d, offs, lens = _arena(blobs, align, shift)
    res = parse_tree_nodes(d, offs, lens, guard=GUARD)
    m = model.records(blobs, offs)
    _compare(res, m.status, m.blobs, b"".join(m.data_ids), b"".join(m.tree_ids),
             np.array(m.is_dir, np.uint8), model.node_array(m.nodes))
    return res, m, (d, offs, lens)


def _compare(res, status, blobs, data_ids, tree_ids, is_dir, want):
    """Every output of a call against what is expected: the statuses, the six
    fields per blob (rows of ``blobs``), the id arrays' bytes, ``is_dir`` and
    the TR_NODE array ``want``; behind them the 0xA5 fill and guard."""
    assert np.array_equal(res.blobs["status"], np.asarray(status))
    got = np.stack([res.blobs[k].astype(np.int64) for k in ("nodes", "data_ids", "tree_ids", "data_start",
                                                            "tree_start", "node_start")], 1)
    assert np.array_equal(got, np.asarray(blobs, np.int64).reshape(-1, 6))
    nd, nt, nn = len(data_ids) // 32, len(tree_ids) // 32, len(want)
    assert (res.n_data_ids, res.n_tree_ids, res.nodes) == (nd, nt, nn)
    assert res.data_ids.cpu().numpy().tobytes() == bytes(data_ids)
    assert res.tree_ids.cpu().numpy().tobytes() == bytes(tree_ids)
    assert np.array_equal(res.tree_is_dir.cpu().numpy(), is_dir)
    assert tuple(res.node_records.shape) == (nn, 32)
    have = res.nodes_host()
    for k in want.dtype.names:
        assert np.array_equal(have[k], want[k]), k
    for flat, used in zip(res.raw, (nd * 32, nt * 32, nt, nn * 32)):
        assert (flat[used:].cpu().numpy() == 0xA5).all()
        assert int(flat.numel()) >= used + GUARD


def test_case_table(gpu_ctx):
    """The extended table in one batch, blobs outside G_N between blobs
    inside it; the same batch through rcdc_tree_parse gives what it gave
    before: there the dir cases are NOT_PARSED, here they are OK."""
    from rustic_core_amd.tree import parse_trees
    yes = [c for c in model.TABLE if c[3]]
    no = [c for c in model.TABLE if not c[3]]
    order = []
    for i in range(max(len(yes), len(no))):
        order += yes[i:i + 1] + no[i:i + 1]
    assert len(order) == len(model.TABLE)
    res, m, (d, offs, lens) = _check([c[1] for c in order], align=1, shift=5)
    assert m.status == [0 if c[3] else 1 for c in order]
    old = parse_trees(d, offs, lens)
    mt = gt.collect([c[1] for c in order])
    assert old.blobs["status"].tolist() == mt.status == [0 if c[2] else 1 for c in order]
    assert old.data_ids.cpu().numpy().tobytes() == b"".join(mt.data_ids)
    assert old.tree_ids.cpu().numpy().tobytes() == b"".join(mt.tree_ids)
    assert old.tree_is_dir.cpu().numpy().tolist() == mt.is_dir
    flip = [c[0] for c, a, b in zip(order, mt.status, m.status) if a != b]
    assert sorted(flip) == sorted(c[0] for c in model.TABLE if c[2] != c[3]) and len(flip) >= 5
    # a blob outside G_N between two others changes nothing of theirs; one blob alone
    _check([c[1] for c in yes], align=16)
    _check([yes[0][1]])
    _check([c[1] for c in no][:3])


_EDGE = serialize(tree(dict(file_node("NAME", [1, 2]), user="u"), dir_node("after", 7))) \
    .replace(b"NAME", b'ab\\"cd')
_ITEMS = {
    "opening_quote": _EDGE.index(b'"ab\\'),
    "escaped_quote": _EDGE.index(b'\\"cd') + 1,
    "closing_quote": _EDGE.index(b'cd"') + 2,
}


def test_name_at_tile_edges(gpu_ctx):
    """A name's opening quote, the escaped quote inside it and its closing
    quote 1 byte before, on and 1 byte after a tile boundary, the arena
    starting 0, 1, 15, 16 and 17 bytes past a 16-byte boundary."""
    from rustic_core_amd.tree import parse_tile
    tile = parse_tile()
    assert model.in_gn(_EDGE) and [_EDGE[i] for i in _ITEMS.values()] == [0x22] * 3
    assert model.name_spans(_EDGE)[0] == (_ITEMS["opening_quote"] + 1, 6, True)
    for shift in (0, 1, 15, 16, 17):
        edge = tile - shift % 16
        blobs = [b" " * (edge + d - at) + _EDGE for at in _ITEMS.values() for d in (-1, 0, 1)]
        res, m, _ = _check(blobs, align=tile, shift=shift)
        assert m.status == [0] * 9 and len(m.nodes) == 18
        assert res.nodes_host()["flags"][::2].tolist() == [model.CONTENT | model.NAME_ESC] * 9


def _node(i, n_ids=None):
    if i % 5 == 0:
        return dir_node(f"d{i}", i % 256)
    if i % 5 == 1:
        return file_node(f"f{i}", [(i + j) % 256 for j in range(i % 4 if n_ids is None else n_ids)])
    if i % 5 == 2:
        return {"name": f"n{i}", "type": "dir"} if i % 2 else {"name": f"e\\{i}", "type": "file"}
    if i % 5 == 3:
        return dict(other_node(f"o{i}", "symlink"), subtree=hid(i % 256) if i % 2 else None)
    return dict(other_node("é" * (i % 7), "fifo"), content=[hid(i % 256)])


def test_counts_around_a_wave_and_a_workgroup(gpu_ctx):
    """63, 64, 65 and 257 nodes in a blob, a file of 4097 ids, 1 and 257
    blobs: across the waves of the numbering's scan.  Every call here holds
    fewer than 1024 nodes, one workgroup of the numbering; more than one is
    ``test_numbering_over_workgroups``, more than one round of their sums
    ``test_numbering_past_a_round_of_sums``."""
    blobs = [serialize(tree(*[_node(i) for i in range(n)])) for n in (63, 64, 65, 257, 0)]
    blobs.append(serialize(tree(file_node("before", [1]), file_node("big", [j % 256 for j in range(4097)]),
                                {"name": "after", "type": "dir"})))
    res, m, _ = _check(blobs, align=1, shift=3)
    assert m.status == [0] * len(blobs) and 64 * 4 < len(m.nodes) < 1024
    assert [b[0] for b in m.blobs] == [63, 64, 65, 257, 0, 3]
    assert m.nodes[-1][3] == len(m.data_ids) and m.nodes[-2][4] == 4097
    _check(blobs[3:4])
    bad = [c[1] for c in model.TABLE if not c[3]]
    many = [bad[i % len(bad)] if i % 5 == 2 else serialize(tree(*[_node(i + k) for k in range(i % 9)]))
            for i in range(257)]
    res, m, _ = _check(many, align=1, shift=9)
    assert sum(m.status) == 51 and len(m.nodes) > 700


@pytest.mark.parametrize("n", (1025, 2049))
def test_numbering_over_workgroups(gpu_ctx, n):
    """``n`` node records from one call: the numbering runs in two and in
    three workgroups of 1024 nodes, and their sums are added back.  Blobs
    outside G_N, whose nodes are counted by no record, stand before and after
    the 1024th node of every workgroup's edge."""
    by_name = {c[0]: c[1] for c in model.TABLE}
    bad = [by_name["unknown_key"],
           serialize(tree(_node(1), _node(5), {"name": "z", "type": "file", "bogus": 1}, _node(6)))]
    assert not any(model.in_gn(b) for b in bad)
    blob = lambda first, count: serialize(tree(*[_node(first + i) for i in range(count)]))
    blobs = [blob(0, 700), bad[0], blob(700, 300), bad[1], blob(1000, 24), bad[0], blob(1024, 1)]
    if n == 2049:
        blobs += [bad[1], blob(1025, 1000), bad[0], blob(2025, 23), bad[1], blob(2048, 1)]
    res, m, _ = _check(blobs, align=1, shift=7)
    assert len(m.nodes) == n and (n - 1) // 1024 == (1 if n == 1025 else 2)
    assert sum(m.status) == (3 if n == 1025 else 6)
    # the parser numbers every node of the text, the rejected blobs' too: they shift
    # a node's place in its workgroup, not its record
    assert res.nodes == n and [b[5] for b in m.blobs][-1] == n - 1


def test_more_tiles_than_a_scan_round(gpu_ctx):
    """tests/test_gpu_tree_parse.py's test of this name through
    rcdc_tree_nodes: 2 100 blobs, more than 2 048 tiles, three rounds of the
    scan over the tiles' counts."""
    from rustic_core_amd.tree import parse_tile
    tile = parse_tile()
    at = _ITEMS["escaped_quote"]
    assert _EDGE[at - 1:at + 1] == b'\\"'
    blobs = _many_tile_blobs(_node, _EDGE, at, [c[1] for c in model.TABLE if not c[3]], tile)
    offs, lens, _ = _arena_layout(blobs, tile)
    assert len(blobs) >= 2100 and _tiles(offs, lens, tile) > 2 * 1024
    res, m, _ = _check(blobs, align=tile)
    assert 20 <= sum(m.status) < 40 and len(m.nodes) > 4000
    assert sum(bool(nd[7] & model.NAME_ESC) for nd in m.nodes) >= 40


def test_a_blob_of_three_state_rounds(gpu_ctx):
    """tests/test_gpu_tree_parse.py's blobs of more than 128 tiles through
    rcdc_tree_nodes: the names behind the long file and behind the string
    that crosses the second round's edge are where the model finds them."""
    from rustic_core_amd.tree import parse_tile
    tile = parse_tile()
    blobs = _long_blobs(tile)
    res, m, _ = _check(blobs, align=tile)
    assert m.status == [0, 0] and [b[0] for b in m.blobs] == [5, 4]
    m_offs, _, _ = _arena_layout(blobs, tile)
    raw = lambda b, nd: blobs[b][nd[0] - m_offs[b]:nd[0] - m_offs[b] + nd[1]]
    assert [raw(0, nd) for nd in m.nodes[:5]] == [b"big", b'q\\"uote', b"]}[{", b"back\\\\slash", b"last"]
    assert [raw(1, nd) for nd in m.nodes[5:]] == [b"big", b"f", b"d", b"g"]


def test_numbering_past_a_round_of_sums(gpu_ctx):
    """2^20 + 2100 node records in one call, and the nodes of two rejected
    blobs besides: 1 029 workgroups number them, so the one workgroup over
    their sums (``block_scan4``) takes a second round with a carry.  The
    blobs and every expected output are tests/tree_numbering_cases.py's
    arithmetic, held to the models by tests/test_tree_numbering_host.py.  A
    rejected blob stands before the 2^20th node and one behind it; the same
    arena through rcdc_tree_parse gives the same but for the records."""
    from rustic_core_amd.tree import parse_tree_nodes, parse_trees
    from tests import tree_numbering_cases as cases
    counts = [32001 + 37 * i for i in range(31)]
    counts = counts[:5] + [1001] + counts[5:] + [40000, 999, 1440]
    bad = [0] * len(counts)
    bad[5], bad[-2] = cases.BAD_KEY, cases.BAD_END
    before = np.cumsum(counts) - counts
    assert before[5] + counts[5] < 1 << 20 < before[-2] and before[-3] < 1 << 20
    e = cases.Expected(counts, bad, align=16)
    assert len(e.nodes) == (1 << 20) + 2100 and len(e.nodes) > 1024 * 1024
    assert sum(len(t) for t in e.texts) < 64 << 20
    d, offs, lens = _arena(e.texts, align=16)
    assert offs == e.offs
    res = parse_tree_nodes(d, offs, lens, guard=GUARD)
    _compare(res, e.status, e.blobs, e.data_ids, e.tree_ids, e.is_dir, e.nodes)
    old = parse_trees(d, offs, lens, guard=GUARD)
    assert np.array_equal(old.blobs["status"], e.status)
    for k, col in zip(("nodes", "data_ids", "tree_ids", "data_start", "tree_start"), e.blobs.T):
        assert np.array_equal(old.blobs[k].astype(np.int64), col), k
    assert (old.n_data_ids, old.n_tree_ids, old.nodes) == (len(e.data_ids) // 32, len(e.tree_ids) // 32,
                                                           len(e.nodes))
    assert old.data_ids.cpu().numpy().tobytes() == e.data_ids
    assert old.tree_ids.cpu().numpy().tobytes() == e.tree_ids
    assert np.array_equal(old.tree_is_dir.cpu().numpy(), e.is_dir)
    for flat, used in zip(old.raw, (len(e.data_ids), len(e.tree_ids), len(e.is_dir))):
        assert (flat[used:].cpu().numpy() == 0xA5).all() and int(flat.numel()) >= used + GUARD


def test_random_trees(gpu_ctx):
    """200 random trees, a tenth with one bit flipped, every fourth dir
    stripped of its subtree: the model decides what is inside G_N."""
    rng = random.Random(2025)
    blobs = []
    for i in range(200):
        o = random_tree(rng)
        for k, n in enumerate(o["nodes"] or []):
            if n["type"] == "dir" and (i + k) % 4 == 0:
                del n["subtree"]
        text = random_text(o, rng)
        blobs.append(flipped(text, rng) if i % 10 == 7 else text)
    res, m, _ = _check(blobs, align=1, shift=13)
    assert 0 < sum(m.status) <= 20 and len(m.nodes) > 300
    assert sum(1 for n in m.nodes if n[6] == 1 and not n[7] & model.SUBTREE) > 10
    assert sum(not gt.in_gt(b) for b in blobs) > sum(m.status) + 10


def test_capacities(gpu_ctx):
    """Capacities at exactly the bound are accepted (``_check`` runs with
    them); one below, each in turn, is refused."""
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.tree import parse_bound, parse_tree_nodes
    text = serialize(tree(file_node("f", [1, 2]), dir_node("d", 3), {"name": "e", "type": "dir"}))
    d, offs, lens = _arena([text])
    bd, bt, bn = parse_bound(len(text))
    res = parse_tree_nodes(d, offs, lens, caps=(bd, bt, bn), guard=GUARD)
    assert (res.n_data_ids, res.n_tree_ids, res.nodes) == (2, 1, 3)
    assert int(res.raw[3].numel()) == bn * 32 + GUARD
    for caps in ((bd - 1, bt, bn), (bd, bt - 1, bn), (bd, bt, bn - 1)):
        with pytest.raises(RusticError) as e:
            parse_tree_nodes(d, offs, lens, caps=caps)
        assert e.value.kind == ErrorKind.InvalidInput and "below" in str(e.value)
    empty = parse_tree_nodes(d, [], [])
    assert empty.nodes == 0 and tuple(empty.node_records.shape) == (0, 32)


# ---- rcdc_tree_names -----------------------------------------------------------------------

_LENGTHS = (0, 1, 15, 16, 17, 300, 2, 3, 5, 7, 11, 13, 33, 64, 4)


def test_names(gpu_ctx):
    """Names of 0, 1, 15, 16, 17 and 300 bytes among others, the source at
    every alignment (the arena's start moves) and the destination at every
    alignment (the names before it differ in length); an empty list, a list
    with repeats, and the guard bytes behind the names."""
    import torch
    from rustic_core_amd.tree import parse_tree_nodes, tree_names
    names = ["".join(chr(97 + (i + k) % 26) for k in range(n)) for i, n in enumerate(_LENGTHS)]
    text = serialize(tree(*[{"name": "N%02d" % i, "type": "fifo"} for i in range(len(names))]))
    for i, nm in enumerate(names):
        text = text.replace(b"N%02d" % i, nm.encode())
    assert model.in_gn(text) and [s[1] for s in model.name_spans(text)] == list(_LENGTHS)
    big = _LENGTHS.index(300)
    lists = [list(range(len(names))), list(range(len(names)))[::-1], [big], [1, 1, big, big, 0, big],
             [1, 1, 1, big], [6, 6, 6, 6, big], []]
    src_al, dst_al, vector = set(), set(), 0
    for shift in range(16):
        d, offs, lens = _arena([b" " * 7, text], shift=shift)
        res = parse_tree_nodes(d, offs, lens)
        host = d.cpu().numpy().tobytes()
        spans = [(offs[1] + a, n) for a, n, _ in model.name_spans(text)]
        for idx in lists:
            index = torch.tensor(idx, dtype=torch.int32, device="cuda:0")
            offsets, flat = tree_names(d, res.node_records, index, guard=GUARD)
            want = [host[a:a + n] for a, n in (spans[i] for i in idx)]
            o = offsets.cpu().numpy().tolist()
            assert o == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
            got = flat.cpu().numpy()
            assert got[:o[-1]].tobytes() == b"".join(want)
            assert (got[o[-1]:] == 0xA5).all() and len(got) >= o[-1] + GUARD
            for i, at in zip(idx, o):
                s, t = d.data_ptr() + spans[i][0], flat.data_ptr() + at
                src_al.add(s % 16)
                dst_al.add(t % 16)
                vector += (s - t) % 16 == 0 and spans[i][1] >= 48
    assert src_al == set(range(16)) and dst_al == set(range(16)) and vector >= 8
    # an index past the records counts as an empty name
    index = torch.tensor([0, 99, 5], dtype=torch.int32, device="cuda:0")
    offsets, flat = tree_names(d, res.node_records, index)
    assert offsets.cpu().numpy().tolist() == [0, 0, 0, 300] and int(flat.numel()) == 300
