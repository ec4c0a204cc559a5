"""Tree blobs of a fixed pattern, large enough for the numbering of
rcdc_tree_nodes to take a second round over its workgroups' sums (more than
2^20 nodes in one call), with every expected output computed by numpy
arithmetic on the pattern's parameters: tests/tree_nodes_model.py takes most
of a minute at that size.  tests/test_tree_numbering_host.py holds the
arithmetic to that model and to tests/tree_json_model.py at a small size.

A blob is ``{"nodes":[`` node ``,`` node ... ``]}``.  Node l of a blob is a
file with one content id where l % 16 == 0, a dir with a subtree where
l % 16 == 8, and ``{"name":"n","type":"fifo","content":null}`` elsewhere.  An
id is 32 bytes that depend on the node's number among all nodes of the call.
A blob outside the grammars keeps all its nodes and differs in a few bytes:
an unknown key (``"tyqe"``) in one node, or no closing brace of the root.
"""
import numpy as np

from tests.tree_nodes_model import CONTENT, SUBTREE

PERIOD = 16
HEAD, TAIL = b'{"nodes":[', b"]}"
FIFO = b'{"name":"n","type":"fifo","content":null}'
FILE = b'{"name":"n","type":"file","content":["' + b"0" * 64 + b'"]}'
DIR = b'{"name":"n","type":"dir","subtree":"' + b"0" * 64 + b'"}'
NAME_AT = len(b'{"name":"')                 # the name's first byte in a node
FILE_ID_AT, DIR_ID_AT = FILE.index(b"0" * 64), DIR.index(b"0" * 64)
BAD_KEY, BAD_END = 1, 2                     # how a blob leaves the grammars
_HEX = np.frombuffer(b"0123456789abcdef", np.uint8)


def _kind_texts():
    return [FILE if l == 0 else DIR if l == 8 else FIFO for l in range(PERIOD)]


def node_ids(g):
    """The 32 id bytes of the nodes numbered ``g`` among all of the call."""
    g = np.asarray(g, np.uint64)[:, None]
    k = np.arange(32, dtype=np.uint64)[None, :]
    return ((g * np.uint64(2654435761) >> (k % np.uint64(24))) + k * np.uint64(37) + np.uint64(1)) \
        .astype(np.uint8)


def _hex(ids):
    return _HEX[np.stack([ids >> 4, ids & 15], 2).reshape(len(ids), 64)]


def blob_text(n, g0, bad=0):
    """The text of a blob of ``n`` nodes, the first of them number ``g0`` of
    the call, and the offsets of its nodes in it."""
    texts = _kind_texts()
    one = np.frombuffer(b"".join(t + b"," for t in texts), np.uint8)
    in_period = np.concatenate([[0], np.cumsum([len(t) + 1 for t in texts])])
    l = np.arange(n)
    at = len(HEAD) + (l // PERIOD) * int(in_period[-1]) + in_period[l % PERIOD]
    body = np.tile(one, n // PERIOD + 1)[:(int(at[-1]) - len(HEAD) + len(texts[(n - 1) % PERIOD])) if n else 0]
    out = np.concatenate([np.frombuffer(HEAD, np.uint8), body, np.frombuffer(TAIL, np.uint8)]).copy()
    for first, id_at in ((0, FILE_ID_AT), (8, DIR_ID_AT)):
        sel = l[l % PERIOD == first]
        if len(sel):
            out[(at[sel] + id_at)[:, None] + np.arange(64)[None, :]] = _hex(node_ids(g0 + sel))
    if bad == BAD_KEY:
        k = int(at[n // 2]) + FIFO.index(b"type")
        assert n // 2 % 8 and bytes(out[k:k + 4]) == b"type"
        out[k + 2] = ord("q")
    elif bad == BAD_END:
        out[-1] = ord(" ")
    return out.tobytes(), at


class Expected:
    """What rcdc_tree_nodes gives for blobs of ``counts`` nodes at ``offs``
    of the arena, ``bad`` (0, BAD_KEY or BAD_END) per blob; ``texts`` are the
    blobs.  ``status``, ``blobs`` (six fields a row), ``data_ids``,
    ``tree_ids`` (bytes), ``is_dir`` and ``nodes`` (a TR_NODE array)."""

    def __init__(self, counts, bad, align=16):
        from rustic_core_amd.tree import TR_NODE
        counts, bad = np.asarray(counts, np.int64), np.asarray(bad, np.int64)
        g0 = np.cumsum(counts) - counts  # every node of the text has a number, parsed or not
        self.texts, ats = [], []
        for n, g, how in zip(counts, g0, bad):
            text, at = blob_text(int(n), int(g), int(how))
            self.texts.append(text)
            ats.append(at)
        lens = np.array([len(t) for t in self.texts], np.int64)
        self.offs, o = [], 0
        for n in lens:  # tests/test_gpu_tree_parse.py ``_arena`` with this ``align`` (not 1)
            o = (o + align - 1) // align * align
            self.offs.append(o)
            o += int(n)
        ok = bad == 0
        files, dirs = (counts + 15) // 16 * ok, (counts + 7) // 16 * ok
        kept = counts * ok
        self.status = (~ok).astype(np.int64)
        d0, t0, n0 = (np.cumsum(x) - x for x in (files, dirs, kept))
        self.blobs = np.stack([kept, files, dirs, d0, t0, n0], 1)
        self.nodes = np.zeros(int(kept.sum()), TR_NODE)
        rec = self.nodes
        b = np.repeat(np.arange(len(counts)), kept)
        l = np.arange(len(b)) - np.repeat(n0, kept)
        rec["name_off"] = np.repeat(np.asarray(self.offs, np.int64), kept) + NAME_AT + \
            (np.concatenate([a for a, k in zip(ats, ok) if k]) if len(b) else 0)
        rec["name_len"], rec["blob"] = 1, b
        rec["data_start"] = d0[b] + (l + 15) // 16
        rec["tree_index"] = t0[b] + (l + 7) // 16
        rec["n_content"] = l % 16 == 0
        rec["type"] = np.where(l % 16 == 0, 0, np.where(l % 16 == 8, 1, 5))
        rec["flags"] = np.where(l % 16 == 0, CONTENT, np.where(l % 16 == 8, SUBTREE, 0))
        g = g0[b] + l
        self.data_ids = node_ids(g[l % 16 == 0]).tobytes()
        self.tree_ids = node_ids(g[l % 16 == 8]).tobytes()
        self.is_dir = np.ones(int(dirs.sum()), np.uint8)
