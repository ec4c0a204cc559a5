"""The node records of rcdc_tree_nodes (include/rcdc.h) in plain Python: the
grammar G_N, which is G_T (tests/tree_json_model.py) with the dir rule
dropped, the facts of a node over ``json.loads``, and the span of its raw
name by a small scanner that reads bytes.  Also the cases the node records
add to the table of tests/tree_json_cases.py, and the level rule of
rcdc_check_trees_level written over the records.

``in_gn(data)``; ``records(blobs, offs)`` -> what a batch gives: statuses,
per-blob counts and starts, the id arrays and a TR_NODE array.
"""
import json

import numpy as np

from tests import tree_json_model as gt
from tests.index_json_cases import hid
from tests.tree_json_cases import CASES, _named, dir_node, file_node, serialize, tree

TYPES = ("file", "dir", "symlink", "dev", "chardev", "fifo", "socket")
CONTENT, SUBTREE, NAME_ESC = 1, 2, 4


class _PN(gt._P):
    """G_T's recogniser with G_N's node: the same members, and a dir may lack
    its subtree."""

    def node(self) -> None:
        v = {}

        def member(k):
            if k in (b"name", b"linktarget"):
                self.string()
            elif k == b"type":
                for t in gt.TYPES:
                    if self.at(b'"' + t + b'"'):
                        v[k] = t
                        return
                raise gt._Outside("type")
            elif k in gt.NULL_OR_U32:
                self.null_or(lambda: self.uint(gt.U32_MAX))
            elif k in gt.NULL_OR_STRING:
                self.null_or(self.string)
            elif k in gt.U64:
                self.uint(gt.U64_MAX)
            elif k == b"content":
                self.null_or(lambda: self.array(self.id))
            elif k == b"subtree":
                self.null_or(self.id)
            else:
                self.array(self.xattr)
        seen = self.members(gt.NODE_KEYS, member)
        if not {b"name", b"type"} <= seen:
            raise gt._Outside("node lacks a key")
        if v[b"type"] == b"symlink" and b"linktarget" not in seen:
            raise gt._Outside("symlink without linktarget")


def in_gn(data: bytes) -> bool:
    try:
        _PN(data).root()
        return True
    except (gt._Outside, IndexError):
        return False


def name_spans(data: bytes):
    """[(offset of the first byte after the opening quote, raw length, holds
    a backslash)] of the "name" of every node of a blob in G_N: strings are
    followed from quote to quote, a string before a ':' is a key, and the
    value after the key ``name`` of an object three brackets deep is a name."""
    d, i, depth, out, want = bytes(data), 0, 0, [], False
    while i < len(d):
        c = d[i]
        if c in b"{[":
            depth += 1
        elif c in b"}]":
            depth -= 1
        elif c == 0x22:
            j = i + 1
            while d[j] != 0x22:
                j += 2 if d[j] == 0x5C else 1
            k = j + 1
            while k < len(d) and d[k] in gt.WS:
                k += 1
            if k < len(d) and d[k] == 0x3A:  # a key
                want = depth == 3 and d[i + 1:j] == b"name"
            elif want:
                out.append((i + 1, j - i - 1, 0x5C in d[i + 1:j]))
                want = False
            i = j
        i += 1
    return out


def node_facts(data: bytes):
    """Per node of a blob that is JSON of the tree shape: (type index,
    content: None or the ids, subtree: None or the id)."""
    out = []
    for n in json.loads(bytes(data).decode("utf-8"))["nodes"] or []:
        c, s = n.get("content"), n.get("subtree")
        out.append((TYPES.index(n["type"]), None if c is None else [bytes.fromhex(i) for i in c],
                    None if s is None else bytes.fromhex(s)))
    return out


class Records:
    """What rcdc_tree_nodes gives for a batch."""

    def __init__(self):
        self.status = []   # per blob: 0 parsed, 1 not parsed
        self.blobs = []    # per blob: (nodes, data_ids, tree_ids, data_start, tree_start, node_start)
        self.data_ids, self.tree_ids, self.is_dir = [], [], []
        self.nodes = []    # TR_NODE fields as tuples


def records(blobs, offs=None) -> Records:
    out = Records()
    offs = [0] * len(blobs) if offs is None else offs
    for b, (data, off) in enumerate(zip(blobs, offs)):
        d0, t0, n0 = len(out.data_ids), len(out.tree_ids), len(out.nodes)
        if not in_gn(data):
            out.status.append(1)
            out.blobs.append((0, 0, 0, d0, t0, n0))
            continue
        facts, spans = node_facts(data), name_spans(data)
        assert len(facts) == len(spans)
        for (tpe, content, subtree), (at, ln, esc) in zip(facts, spans):
            flags = (CONTENT if content is not None else 0) | (SUBTREE if subtree is not None else 0) \
                | (NAME_ESC if esc else 0)
            out.nodes.append((off + at, ln, b, len(out.data_ids), len(content or []),
                              len(out.tree_ids), tpe, flags, 0))
            if tpe == 0:
                out.data_ids += content or []
            if subtree is not None:
                out.tree_ids.append(subtree)
                out.is_dir.append(int(tpe == 1))
        out.status.append(0)
        out.blobs.append((len(facts), len(out.data_ids) - d0, len(out.tree_ids) - t0, d0, t0, n0))
    return out


def node_array(nodes) -> np.ndarray:
    from rustic_core_amd.tree import TR_NODE
    return np.array(nodes, TR_NODE) if nodes else np.zeros(0, TR_NODE)


# ---- the cases the node records add: (name, bytes, in G_T, in G_N) ---------------

def _extra():
    f = lambda **kw: dict({"name": "f", "type": "file"}, **kw)
    out = [
        ("gn_dir_without_subtree", serialize(tree({"name": "d", "type": "dir"})), False, True),
        ("gn_dir_subtree_null", serialize(tree({"name": "d", "type": "dir", "subtree": None},
                                               dir_node("e", 3))), False, True),
        ("gn_dir_without_subtree_between", serialize(tree(
            file_node("a", [1, 2]), {"name": "d", "type": "dir", "content": None},
            dir_node("e", 3), file_node("b", [4]))), False, True),
        ("gn_file_without_content", serialize(tree(f())), True, True),
        ("gn_file_content_null", serialize(tree(f(content=None))), True, True),
        ("gn_file_content_empty", serialize(tree(f(content=[]))), True, True),
        ("gn_three_contents", serialize(tree(f(), f(content=None), f(content=[]),
                                             file_node("g", [1, 2]), f(content=[]))), True, True),
        ("gn_name_empty", _named(b""), True, True),
        ("gn_name_escaped_quote", _named(b'a\\"b'), True, True),
        ("gn_name_unicode_escape", _named(b"\\u00e9"), True, True),
        ("gn_name_raw_utf8", _named("é€\U0001F600".encode()), True, True),
        ("gn_name_leading_slash", _named(b"/abs/path"), True, True),
        ("gn_name_last_key", serialize(tree({"type": "file", "content": [hid(1)], "name": "last"},
                                            {"type": "dir", "name": "x"})), False, True),
        ("gn_user_named_name", serialize(tree(dict(f(content=[hid(2)]), user="name",
                                                   group='"name":"x"'))), True, True),
        ("gn_xattr_named_name", serialize(tree(dict(
            {"type": "file"}, extended_attributes=[{"name": "name", "value": None}], name="real"))),
         True, True),
    ]
    return out


EXTRA = _extra()
# the whole table: G_T's cases are inside G_N exactly where they are inside G_T, but for
# the two dir cases
TABLE = [(n, d, g, g or n in ("dir_without_subtree", "dir_subtree_null")) for n, d, g in CASES] + EXTRA
assert len({c[0] for c in TABLE}) == len(TABLE)


# ---- the level rule over records --------------------------------------------------

KINDS = ("FileHasNoContent", "FileBlobHasNullId", "FileBlobNotInIndex", "NoSubTree", "NullSubTree",
         "SubTreeMissingInIndex")
NO_PACK = 0xFFFFFFFF


def level_rule(nodes, data_ids, data_hits, tree_ids, tree_hits):
    """check_trees' rule over node records (tuples in TR_NODE's order), ids
    (bytes) and hits ((count, pack) per id): ([(node, kind, blob_num)], the
    data packs marked, the tree packs marked)."""
    null = bytes(32)
    miss = lambda h: h[0] == 0 or h[1] == NO_PACK
    found, dp, tp = [], set(), set()
    for k, (_, _, _, d0, nc, t, tpe, flags, _) in enumerate(nodes):
        if tpe == 0:
            if not flags & CONTENT:
                found.append((k, 0, 0))
            for i in range(nc if flags & CONTENT else 0):
                if data_ids[d0 + i] == null:
                    found.append((k, 1, i))
                if miss(data_hits[d0 + i]):
                    found.append((k, 2, i))
                else:
                    dp.add(data_hits[d0 + i][1])
        elif tpe == 1:
            if not flags & SUBTREE:
                found.append((k, 3, 0))
            elif tree_ids[t] == null:
                found.append((k, 4, 0))
            elif miss(tree_hits[t]):
                found.append((k, 5, 0))
            else:
                tp.add(tree_hits[t][1])
    return found, dp, tp


def level_rule_np(nodes, data_ids, data_hits, tree_ids, tree_hits):
    """``level_rule`` in numpy, for levels too large for it (held to it by
    tests/test_tree_nodes_host.py): ``nodes`` a TR_NODE array, the ids (n, 32)
    uint8, the hits (n, 2) arrays of (count, pack).  Returns the findings as an
    (n, 3) int64 array of (node, kind, blob_num) in the rule's order, and the
    two sets of marked packs."""
    tpe, flags = nodes["type"], nodes["flags"]
    d0, nc = nodes["data_start"].astype(np.int64), nodes["n_content"].astype(np.int64)
    data_hits = np.asarray(data_hits, np.int64).reshape(-1, 2)
    tree_hits = np.asarray(tree_hits, np.int64).reshape(-1, 2)
    miss = lambda h: (h[:, 0] == 0) | (h[:, 1] == NO_PACK)
    # per id of the arrays once, then picked per judged id: no row is copied
    is_null = lambda ids: ~np.ascontiguousarray(ids).view(np.uint64).reshape(-1, 4).any(1) \
        if len(ids) else np.zeros(0, bool)
    k_all = np.arange(len(nodes), dtype=np.int64)
    rows = []  # (node, blob_num, kind): the rule's order is this tuple's

    def add(k, num, kind):
        rows.append(np.stack([k, num, np.full(len(k), kind, np.int64)], 1))
    files = tpe == 0
    with_content = files & ((flags & CONTENT) != 0)
    k = k_all[files & ~with_content]
    add(k, np.zeros(len(k), np.int64), 0)
    k, n = k_all[with_content], nc[with_content]
    of_id = np.repeat(k, n)                                    # the node of every judged id
    num = np.arange(len(of_id), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    at = np.repeat(d0[with_content], n) + num
    null, lacks = is_null(data_ids)[at], miss(data_hits)[at]
    add(of_id[null], num[null], 1)
    add(of_id[lacks], num[lacks], 2)
    dp = set(np.unique(data_hits[:, 1][at[~lacks]]).tolist())
    dirs = tpe == 1
    with_sub = dirs & ((flags & SUBTREE) != 0)
    k = k_all[dirs & ~with_sub]
    add(k, np.zeros(len(k), np.int64), 3)
    k, t = k_all[with_sub], nodes["tree_index"][with_sub].astype(np.int64)
    null = is_null(tree_ids)[t]
    lacks = ~null & miss(tree_hits)[t]
    add(k[null], np.zeros(int(null.sum()), np.int64), 4)
    add(k[lacks], np.zeros(int(lacks.sum()), np.int64), 5)
    tp = set(np.unique(tree_hits[:, 1][t[~null & ~lacks]]).tolist())
    found = np.concatenate(rows)
    found = found[np.lexsort((found[:, 2], found[:, 1], found[:, 0]))]
    return found[:, [0, 2, 1]], dp, tp


# Tree blobs of the reference's recorded check repositories (tests/check_cases.py) that
# lie outside G_N, counted by tests/test_tree_nodes_host.py: what the device route of
# check_trees leaves to the host there.
OUTSIDE_GN = {
    "repo-data-missing.tar.gz": 0,
    "repo-duplicates.tar.gz": 0,
    "repo-index-missing-blob.tar.gz": 0,
    "repo-index-missing.tar.gz": 0,   # its snapshot's tree is not in the index: nothing is read
    "repo-mixed.tar.gz": 0,           # the same
    "repo-obsolete-index.tar.gz": 0,
    "repo-unreferenced-data.tar.gz": 0,
    "repo-unused-data-missing.tar.gz": 0,
}
