"""CPU: the arithmetic of tests/tree_numbering_cases.py (what the device test
of more than 2^20 nodes expects) against the models of the two grammars at a
size they handle: three blobs of about 70 nodes, one of them outside the
grammars."""
import numpy as np
import pytest

from tests import tree_json_model as gt
from tests import tree_nodes_model as model
from tests import tree_numbering_cases as cases


@pytest.mark.parametrize("bad", ((0, cases.BAD_KEY, 0), (0, 0, cases.BAD_END), (cases.BAD_KEY, 0, 0),
                                 (0, 0, 0)))
def test_expected_against_the_models(bad):
    counts = (70, 73, 65)
    e = cases.Expected(counts, bad)
    assert [model.in_gn(t) for t in e.texts] == [not b for b in bad]
    assert [gt.in_gt(t) for t in e.texts] == [not b for b in bad]
    m = model.records(e.texts, e.offs)
    assert m.status == e.status.tolist()
    assert m.blobs == [tuple(r) for r in e.blobs.tolist()]
    assert b"".join(m.data_ids) == e.data_ids and b"".join(m.tree_ids) == e.tree_ids
    assert m.is_dir == e.is_dir.tolist()
    want = model.node_array(m.nodes)
    assert len(want) == len(e.nodes) == sum(n for n, b in zip(counts, bad) if not b)
    for k in want.dtype.names:
        assert np.array_equal(want[k], e.nodes[k]), k
    # rcdc_tree_parse's outputs are the same but for the node records
    t = gt.collect(e.texts)
    assert t.status == m.status and t.blobs == [b[:5] for b in m.blobs] and t.nodes == len(m.nodes)
    assert t.data_ids == m.data_ids and t.tree_ids == m.tree_ids and t.is_dir == m.is_dir


def test_texts_and_ids():
    """The pattern: a file at every 16th node, a dir eight behind it, ids
    that differ from node to node; blobs of 0, 1, 8, 9, 16 and 17 nodes."""
    import json
    g = 0
    for n in (0, 1, 8, 9, 16, 17, 40):
        text, at = cases.blob_text(n, g)
        nodes = json.loads(text)["nodes"]
        assert [x["type"] for x in nodes] == \
            ["file" if l % 16 == 0 else "dir" if l % 16 == 8 else "fifo" for l in range(n)]
        assert [text[a:a + 1] for a in at] == [b"{"] * n
        for l, x in enumerate(nodes):
            if l % 8 == 0:
                hexid = x["content"][0] if l % 16 == 0 else x["subtree"]
                assert bytes.fromhex(hexid) == cases.node_ids([g + l])[0].tobytes()
        g += n
    ids = cases.node_ids(np.arange(5000))
    assert len({r.tobytes() for r in ids}) == 5000 and ids.any(1).all()
