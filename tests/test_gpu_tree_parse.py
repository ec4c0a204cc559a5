"""Tree blobs parsed on the device (rcdc_tree_parse, tree.parse_trees) against
the plain-Python model of the grammar G_T (tests/tree_json_model.py)."""
import random

import numpy as np
import pytest

from tests import tree_json_model as model
from tests.index_json_cases import hid
from tests.tree_json_cases import (CASES, dir_node, file_node, flipped, other_node, random_text,
                                   random_tree, serialize, tree)

pytestmark = pytest.mark.gpu

GUARD = 256


def _arena_layout(blobs, align=1):
    """(offs, lens, the arena's length) of ``_arena``."""
    offs, o = [], 0
    for f in blobs:
        o = (o + align - 1) // align * align
        offs.append(o)
        o += len(f) + (1 if align == 1 else 0)
    return offs, [len(f) for f in blobs], o


def _arena(blobs, align=1, shift=0):
    """One device arena holding ``blobs``: each at a multiple of ``align``,
    the whole tensor starting ``shift`` bytes past a 16-byte boundary (0xFF
    between the blobs, so a read past a blob's end does not look like
    whitespace).  Returns (tensor, offs, lens)."""
    import torch
    offs, _, o = _arena_layout(blobs, align)
    host = np.full(o + shift + 1, 0xFF, np.uint8)
    for off, f in zip(offs, blobs):
        host[shift + off:shift + off + len(f)] = np.frombuffer(f, np.uint8)
    t = torch.from_numpy(host).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    return t[shift:shift + o], offs, [len(f) for f in blobs]


def _check(blobs, align=1, shift=0, judged=None):
    """Parse ``blobs`` in one call and compare every output with the model
    over ``judged`` (the blobs themselves unless the test knows better);
    nothing is written past the counts reported (0xA5 fill and guard)."""
    from rustic_core_amd.tree import parse_trees
    d, offs, lens = _arena(blobs, align, shift)
    res = parse_trees(d, offs, lens, guard=GUARD)
    m = model.collect(judged or blobs)
    assert res.blobs["status"].tolist() == m.status
    got = [(int(b["nodes"]), int(b["data_ids"]), int(b["tree_ids"]), int(b["data_start"]),
            int(b["tree_start"])) for b in res.blobs]
    assert got == m.blobs
    nd, nt = len(m.data_ids), len(m.tree_ids)
    assert (res.n_data_ids, res.n_tree_ids, res.nodes) == (nd, nt, m.nodes)
    assert res.data_ids.cpu().numpy().tobytes() == b"".join(m.data_ids)
    assert res.tree_ids.cpu().numpy().tobytes() == b"".join(m.tree_ids)
    assert res.tree_is_dir.cpu().numpy().tolist() == m.is_dir
    for flat, used in zip(res.raw, (nd * 32, nt * 32, nt)):
        assert (flat[used:].cpu().numpy() == 0xA5).all()
        assert int(flat.numel()) >= used + GUARD
    return res, m


def test_case_table(gpu_ctx):
    """The whole table in one batch, accepted and rejected blobs in turns,
    back to back at odd offsets in an arena that starts off a 16-byte
    boundary."""
    from rustic_core_amd.tree import parse_trees
    yes = [c for c in CASES if c[2]]
    no = [c for c in CASES if not c[2]]
    order = []
    for i in range(max(len(yes), len(no))):
        order += yes[i:i + 1] + no[i:i + 1]
    assert len(order) == len(CASES)
    res, m = _check([c[1] for c in order], align=1, shift=5)
    assert m.status == [0 if c[2] else 1 for c in order]
    # a rejected blob between two accepted ones changes nothing of theirs
    res2, m2 = _check([c[1] for c in yes], align=16)
    assert m2.data_ids == m.data_ids and m2.tree_ids == m.tree_ids and m2.is_dir == m.is_dir
    assert res2.data_ids.cpu().numpy().tobytes() == res.data_ids.cpu().numpy().tobytes()
    assert res2.tree_ids.cpu().numpy().tobytes() == res.tree_ids.cpu().numpy().tobytes()
    # and one blob at a time: a blob's verdict does not depend on its neighbours
    _check([yes[0][1]])
    _check([c[1] for c in no][:3])
    # ids counted, not written
    d, offs, lens = _arena([c[1] for c in order])
    cnt = parse_trees(d, offs, lens, want=(False, False))
    assert cnt.data_ids is None and cnt.tree_ids is None and cnt.tree_is_dir is None
    assert (cnt.n_data_ids, cnt.n_tree_ids) == (len(m.data_ids), len(m.tree_ids))
    assert cnt.blobs.tolist() == res.blobs.tolist()
    one = parse_trees(d, offs, lens, want=(False, True))
    assert one.tree_ids.cpu().numpy().tobytes() == b"".join(m.tree_ids)


# A blob with every item of the tile-edge test; each marker is unique in it.
_EDGE = serialize(tree(
    dict(file_node("PLAIN", [1, 2, 3]), user="RUN1"),
    dict(dir_node("ESCQ", 7), user="RUN2", group="RUN3"),
    other_node("last", "fifo"))) \
    .replace(b"ESCQ", b'es\\"cq').replace(b"RUN1", b"r\\n1").replace(b"RUN2", b"r\\\\2") \
    .replace(b"RUN3", b'r\\\\\\"3')
_ITEMS = {
    "quote": _EDGE.index(b'"PLAIN"'),
    "escaped_quote": _EDGE.index(b'\\"cq') + 1,
    "after_backslash_run_of_1": _EDGE.index(b"\\n1") + 1,
    "after_backslash_run_of_2": _EDGE.index(b"\\\\2") + 2,
    "after_backslash_run_of_3": _EDGE.index(b'\\\\\\"3') + 3,
    "content_bracket": _EDGE.index(b'"content":[') + 10,
    "id": _EDGE.index(hid(2).encode()),
    "id_quote": _EDGE.index(hid(3).encode()) - 1,
    "node_brace": _EDGE.index(b'{"name":"es'),
}


def test_tile_edges(gpu_ctx):
    """Every item 1 byte before, on and 1 byte after a tile boundary, with
    the arena starting 0..17 bytes past a 16-byte boundary.  Blobs start at
    multiples of the tile in the arena, so their first tile ends
    tile - (shift % 16) bytes into the blob."""
    from rustic_core_amd.tree import parse_tile
    tile = parse_tile()
    assert model.in_gt(_EDGE) and max(_ITEMS.values()) < tile - 40
    assert _EDGE[_ITEMS["escaped_quote"]] == 0x22 and _EDGE[_ITEMS["content_bracket"]] == 0x5B
    assert _EDGE[_ITEMS["node_brace"]] == 0x7B and _EDGE[_ITEMS["id_quote"]] == 0x22
    one = model.ids_of(_EDGE)
    assert (one[0], len(one[1]), len(one[2])) == (3, 3, 1)
    for shift in range(18):
        edge = tile - shift % 16
        blobs = [b" " * (edge + d - at) + _EDGE for at in _ITEMS.values() for d in (-1, 0, 1)]
        res, m = _check(blobs, align=tile, shift=shift)
        assert m.status == [0] * len(blobs)


def test_backslash_runs_of_a_tile(gpu_ctx):
    """A name of exactly one tile of backslashes that ends at a tile boundary
    is accepted: the look-back sees the whole run.  The same with tile + 2
    backslashes is in G_T as a text and is rejected only by the look-back
    cap; moved so that no boundary sees more than a tile of it, it is
    accepted again."""
    from rustic_core_amd.tree import parse_tile
    tile = parse_tile()
    head = b'{"nodes":[{"name":"'
    tail = b'","type":"file","content":["' + hid(4).encode() + b'"]}]}\n'
    run = lambda n, pad: b" " * pad + head + b"\\" * n + tail
    # the run ends where the third tile begins
    at_edge = lambda n: run(n, 2 * tile - len(head) - n)
    exact = at_edge(tile)
    capped = at_edge(tile + 2)
    capped_moved = run(tile + 2, 2 * tile - len(head) - (tile + 2) + 5)
    odd = at_edge(tile - 1)  # an odd run: the closing quote is escaped, the string goes on
    for b in (exact, capped, capped_moved):
        assert model.in_gt(b)
    assert not model.in_gt(odd)
    blobs = [exact, capped, capped_moved, odd, exact]
    res, m = _check(blobs, align=tile,
                    judged=[exact, b"rejected only by the look-back cap", capped_moved, odd, exact])
    assert m.status == [0, 1, 0, 1, 0]


def _node(i, n_ids=None):
    if i % 3 == 0:
        return dir_node(f"d{i}", i % 256)
    if i % 3 == 1:
        return file_node(f"f{i}", [(i + j) % 256 for j in range(i % 4 if n_ids is None else n_ids)])
    return dict(other_node(f"o{i}", "symlink"), subtree=hid(i % 256) if i % 2 else None)


def test_counts_around_a_wave_and_a_workgroup(gpu_ctx):
    from rustic_core_amd.tree import parse_tile
    blobs = [serialize(tree(*[_node(i) for i in range(n)])) for n in (63, 64, 65, 257, 0)]
    for n in (63, 64, 65, 4097):
        blobs.append(serialize(tree(file_node("big", [j % 256 for j in range(n)]))))
    assert len(blobs[-1]) // parse_tile() == 67  # 67 whole tiles and a ragged one
    res, m = _check(blobs, align=1, shift=3)
    assert m.status == [0] * len(blobs)
    assert [b[0] for b in m.blobs[:5]] == [63, 64, 65, 257, 0]
    assert [b[1] for b in m.blobs[5:]] == [63, 64, 65, 4097]
    # 1 blob and 257 blobs, every fifth outside G_T
    _check(blobs[3:4])
    bad = [c[1] for c in CASES if not c[2]]
    many = [bad[i % len(bad)] if i % 5 == 2 else serialize(tree(*[_node(i + k) for k in range(i % 7)]))
            for i in range(257)]
    res, m = _check(many, align=1, shift=9)
    assert sum(m.status) == 51 and m.nodes > 500


def _tiles(offs, lens, tile, shift=0):
    """The tiles of a call as the parser counts them: a blob's first tile
    starts at the 16-byte boundary at or before its first byte."""
    return sum(((o + shift) % 16 + n + tile - 1) // tile for o, n in zip(offs, lens) if n)


def _many_tile_blobs(node, edge, quote_at, rejected, tile, n=2100):
    """``n`` blobs of a few spaces and a tree of 1 to 3 ``node``s each; every
    50th is ``edge`` moved so that the escaped quote of its name (at
    ``quote_at``) is the first byte of the blob's second tile and its
    backslash the last of the first; every 97th is one of ``rejected``."""
    blobs = []
    for i in range(n):
        if i % 97 == 96:
            blobs.append(rejected[(i // 97) % len(rejected)])
        elif i % 50 == 49:
            blobs.append(b" " * (tile - quote_at) + edge)
        else:
            blobs.append(b" " * (i % 5) + serialize(tree(*[node(i + k) for k in range(1 + i % 3)])))
    return blobs


def test_more_tiles_than_a_scan_round(gpu_ctx):
    """2 100 blobs at multiples of the tile, more than 2 048 tiles: the one
    workgroup that scans the tiles' counts (``block_scan4``) takes three
    rounds of 1024 and carries the totals from round to round.  Blobs of two
    tiles and rejected blobs stand among them, so a tile's rank is not its
    blob's number."""
    from rustic_core_amd.tree import parse_tile
    tile = parse_tile()
    at = _ITEMS["escaped_quote"]
    assert _EDGE[at - 1:at + 1] == b'\\"'
    blobs = _many_tile_blobs(_node, _EDGE, at, [c[1] for c in CASES if not c[2]], tile)
    offs, lens, _ = _arena_layout(blobs, tile)
    assert len(blobs) >= 2100 and _tiles(offs, lens, tile) > 2 * 1024
    assert all(lens[i] > tile for i in range(49, len(blobs), 50) if i % 97 != 96)
    res, m = _check(blobs, align=tile)
    assert 20 <= sum(m.status) < 40 and m.nodes > 4000
    # a rejected blob and a blob of two tiles on either side of both round edges
    first = np.cumsum([0] + [(n + tile - 1) // tile for n in lens])
    for edge in (1024, 2048):
        b = int(np.searchsorted(first, edge, "right")) - 1
        near = range(b - 100, b + 100)
        assert any(m.status[i] for i in near if i < b) and any(m.status[i] for i in near if i > b)
        assert any(lens[i] > tile for i in near if i < b) and any(lens[i] > tile for i in near if i > b)


def _long_blobs(tile):
    """Two blobs of 130 to 140 tiles: a file of 8 400 ids and behind it nodes
    whose names hold an escaped quote, brackets and a backslash; and one in
    which a string (a ``user`` of brackets and escaped quotes) begins in tile
    127 and ends in tile 129, so the state carried into the third round of 64
    tiles is inside a string."""
    ids = [j % 256 for j in range(8400)]
    one = serialize(tree(file_node("big", ids), dict(file_node("NAME1", [1, 2]), user="u"),
                         dir_node("NAME2", 7), dict(file_node("NAME3", [3]), group="g"),
                         other_node("last", "fifo"))) \
        .replace(b"NAME1", b'q\\"uote').replace(b"NAME2", b"]}[{").replace(b"NAME3", b"back\\\\slash")
    head = serialize(tree(file_node("big", ids[:7800]), dict(file_node("f", [5]), user="USER"),
                          dir_node("d", 9), file_node("g", [6, 7])))
    start = head.index(b"USER")
    fill = b'x]}[{\\"y[{' * (2 * tile // 10)
    value = fill[:(129 * tile + 100) - start]
    assert value[-2:-1] != b"\\"  # the value does not end inside an escape
    two = head.replace(b"USER", value)
    assert start // tile == 127 and (start + len(value)) // tile == 129
    return [one, two]


def test_a_blob_of_three_state_rounds(gpu_ctx):
    """``tile_state`` walks a blob's tiles 64 at a time with one wave; these
    blobs have more than 128 tiles, so the state is carried over two round
    edges, the second time out of a carried state."""
    from rustic_core_amd.tree import parse_tile
    tile = parse_tile()
    blobs = _long_blobs(tile)
    for b in blobs:
        assert 130 <= (len(b) + tile - 1) // tile <= 140 and model.in_gt(b)
    res, m = _check(blobs, align=tile)
    assert m.status == [0, 0] and [b[0] for b in m.blobs] == [5, 4]
    assert m.blobs[0][1] == 8400 + 3 and m.blobs[1][1] == 7800 + 3
    # and behind a short blob, off the tile's grid
    _check([blobs[1][-300:], blobs[1], blobs[0]], align=16)


def test_random_trees(gpu_ctx):
    """200 random trees, a tenth with one bit flipped: the model decides what
    a flip leaves inside G_T, nothing is skipped."""
    rng = random.Random(2024)
    blobs = []
    for i in range(200):
        text = random_text(random_tree(rng), rng)
        blobs.append(flipped(text, rng) if i % 10 == 7 else text)
    res, m = _check(blobs, align=1, shift=13)
    assert 0 < sum(m.status) <= 20 and len(m.data_ids) > 100 and len(m.tree_ids) > 50


def test_invalid_input(gpu_ctx):
    import torch
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.tree import parse_bound, parse_trees
    text = serialize(tree(file_node("f", [1, 2]), dir_node("d", 3)))
    d, offs, lens = _arena([text])
    for o, ln in ((0, lens[0] + 8), (int(d.numel()) + 1, 0), (2 ** 63, 1)):
        with pytest.raises(RusticError) as e:
            parse_trees(d, [o], [ln])
        assert e.value.kind == ErrorKind.InvalidInput and "outside the arena" in str(e.value)
    bd, bt, _ = parse_bound(len(text))
    assert bd >= 2 and bt >= 1
    for caps in ((bd - 1, bt), (bd, bt - 1)):
        with pytest.raises(RusticError) as e:
            parse_trees(d, offs, lens, caps=caps)
        assert e.value.kind == ErrorKind.InvalidInput and "below" in str(e.value)
    with pytest.raises(RusticError):
        parse_trees(d.cpu(), offs, lens)
    with pytest.raises(RusticError):
        parse_trees(d, offs, lens + [1])
    # no blobs: nothing is launched
    res = parse_trees(d, [], [])
    assert res.n_data_ids == 0 and len(res.blobs) == 0 and tuple(res.data_ids.shape) == (0, 32)
    empty = parse_trees(torch.empty(0, dtype=torch.uint8, device="cuda:0"), [0], [0])
    assert empty.blobs["status"].tolist() == [1]
