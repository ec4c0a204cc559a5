"""Models for the repair tests: rcdc_repair_trees_level over node records and
rcdc_repair_spread's fixed point, in numpy.  tests/test_repair_host.py holds
both against the Python rule of rustic_core_amd.repair on built repositories.
"""
import numpy as np

NO_EDGE = 0xFFFFFFFF
NO_NODE = 0xFFFFFFFFFFFFFFFF
NO_PACK = 0xFFFFFFFF
F, D = 0, 1
CONTENT, SUBTREE = 1, 2


def level_model(nodes, data_hits, tree_hits, is_dir, blob_slot, n_slots):
    """``nodes``: a TR_NODE array; ``data_hits``: (n, 2) of (count, pack) per
    entry of d_data_ids; ``tree_hits``: (m, 2) of (count, entry) per entry of
    d_tree_ids; ``is_dir``: m flags; ``blob_slot``: the slot per blob.
    Returns (the damaged slots as a sorted list, the (m, 2) uint32 edges,
    (missing ids, damaged nodes, files without content, the lowest of them))."""
    nodes = np.asarray(nodes)
    data_hits = np.asarray(data_hits, np.int64).reshape(-1, 2)
    tree_hits = np.asarray(tree_hits, np.int64).reshape(-1, 2)
    blob_slot = np.asarray(blob_slot, np.int64)
    n_data, n_tree = len(data_hits), len(tree_hits)
    tpe, flags = nodes["type"].astype(np.int64), nodes["flags"].astype(np.int64)
    start, count = nodes["data_start"].astype(np.int64), nodes["n_content"].astype(np.int64)
    blob = nodes["blob"].astype(np.int64)
    slot = np.full(len(nodes), NO_EDGE, np.int64)
    slot[blob < len(blob_slot)] = blob_slot[blob[blob < len(blob_slot)]]
    slot = np.where(slot < n_slots, slot, NO_EDGE)
    # per id: its node is the last record with data_start <= i
    missing = (data_hits[:, 0] == 0) | (data_hits[:, 1] == NO_PACK)
    node_bad = np.zeros(len(nodes), bool)
    n_missing = 0
    if len(nodes) and n_data:
        i = np.arange(n_data)
        k = np.searchsorted(start, i, "right") - 1
        ok = (k >= 0)
        kk = np.maximum(k, 0)
        ok &= (tpe[kk] == F) & (i - start[kk] < count[kk]) & missing
        n_missing = int(ok.sum())
        node_bad[kk[ok]] = True
    no_sub = (tpe == D) & ((flags & SUBTREE) == 0)
    bad = (node_bad & (tpe == F)) | no_sub
    damaged = sorted({int(s) for s in slot[bad] if s != NO_EDGE})
    no_content = (tpe == F) & ((flags & CONTENT) == 0)
    edges = np.full((n_tree, 2), 0xA5A5A5A5, np.uint32)  # an entry no node owns is not written
    for kx in np.nonzero((flags & SUBTREE) != 0)[0]:
        t = int(nodes["tree_index"][kx])
        if t >= n_tree:
            continue
        e = (NO_EDGE, NO_EDGE)
        if is_dir[t] and slot[kx] != NO_EDGE and tree_hits[t, 0] != 0 and tree_hits[t, 1] < n_slots:
            e = (int(slot[kx]), int(tree_hits[t, 1]))
        edges[t] = e
    first = int(np.nonzero(no_content)[0][0]) if no_content.any() else NO_NODE
    return damaged, edges, (n_missing, int(bad.sum()), int(no_content.sum()), first)


def spread_model(edges, damaged):
    """The least fixed point of changed[p] |= changed[c] from ``damaged`` (a
    byte or bool per slot) over ``edges`` ((n, 2) of (parent, child)): a
    uint8 array."""
    changed = np.asarray(damaged).astype(bool).copy()
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    e = e[(e[:, 0] < len(changed)) & (e[:, 1] < len(changed))]
    while True:
        new = changed.copy()
        np.logical_or.at(new, e[:, 0], changed[e[:, 1]])
        if (new == changed).all():
            return changed.astype(np.uint8)
        changed = new
