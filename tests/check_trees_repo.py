"""Repositories for the check_trees tests: tests/used_blobs_repo.py's trees
plus a fourth snapshot whose trees carry every finding of check_trees, packed
with the project's packer and sealing, and a data index that knows the data
blobs by name.

The fourth snapshot ("root3"):
  kinds     a file without content; a file whose ids are [ok, null, missing,
            null]; a dir without a subtree; a dir with an all-zero subtree
            (the index holds an empty tree under that id, so the walk goes
            on); a dir "gone" whose tree an index built ``without`` it lacks
  /abs      a leading '/', over a name with a JSON escape (q"uote), over a
            name with a Go escape (d\\x41 is dA): a file without content three
            levels down, reported as /abs/q"uote/dA/lost
  twice_a,  the same tree twice: its finding is reported under the first
  twice_b
  host      a tree outside the device's grammar (an unknown key) with a
            finding of its own and, in the tree below it, a file whose blob
            the data index lacks
"""
import hashlib
import json

import numpy as np

from tests import used_blobs_repo as ubr

KEY = bytes(range(64))
NULL = bytes(32)
MISSING = ("gone.0", "gone.1")  # data blobs no pack holds


def _file(name, ids=None, **kw):
    o = dict({"name": name, "type": "file"}, **kw)
    if ids is not None:
        o["content"] = [i.hex() if isinstance(i, bytes) else ubr.did(i).hex() for i in ids]
    return o


def build() -> ubr.Repo:
    r = ubr.build()
    d = ubr._dir
    r.trees[NULL] = b'{"nodes":[]}\n'  # what the all-zero subtree leads to
    r.names[NULL] = "null"
    gone = r.add("gone-leaf", [_file("g", ["g.0"])])
    kinds = r.add("kinds", [
        _file("none"), _file("nullcontent", content=None), _file("empty", []),
        _file("four", ["k.0", NULL, MISSING[0], NULL]),
        {"name": "nosub", "type": "dir"}, {"name": "nosub2", "type": "dir", "subtree": None},
        d("nullsub", NULL), d("gone", gone), _file("fine", ["k.1", "shared"]),
        {"name": "pipe", "type": "fifo", "content": [ubr.did(MISSING[1]).hex()]}])
    deep3 = r.add("deep3", [_file("lost"), _file("kept", ["k.2"])])
    deep2 = r.add("deep2", [d("d\\x41", deep3)])
    deep1 = r.add("deep1", [d('q"uote', deep2)])
    twice = r.add("twice", [_file("s", content=None)])
    below = r.add("host-below", [_file("hb", ["hb.0", MISSING[1]])])
    host = r.add("host", [_file("hf"), d("below", below)], extra="generic_attributes")
    r.snapshots = r.snapshots + [r.add("root3", [
        d("kinds", kinds), d("/abs", deep1), d("twice_a", twice), d("twice_b", twice),
        d("host", host)])]
    return r


def data_ids(r: ubr.Repo):
    """Every content id of a file node, but the all-zero id and MISSING."""
    out = {}
    for text in r.trees.values():
        for n in json.loads(text)["nodes"] or []:
            if n["type"] == "file":
                for i in n.get("content") or []:
                    out[bytes.fromhex(i)] = None
    for i in (NULL,) + tuple(ubr.did(m) for m in MISSING):
        out.pop(i, None)
    return list(out)


class Packed:
    """``repo`` in three tree packs made by the device packer, every third
    tree blob a zstd frame of the device encoder (what
    tests/test_gpu_used_blobs.py's Built does for its repository), and its
    data blobs in index packs of 7 that exist by name only."""

    def __init__(self, gpu_ctx, repo: ubr.Repo):
        from rustic_core_amd.crypto import Key
        from rustic_core_amd.index import IndexPack
        from rustic_core_amd.pack import parse_header
        from tests.prune_cases import bid
        from tests.test_gpu_pack import _build
        from tests.test_gpu_zstd_check import _device_frames
        self.repo = r = repo
        self.names = {v: k for k, v in r.names.items()}
        rng = np.random.default_rng(5)
        ids = list(r.trees)
        texts = [r.trees[i] for i in ids]
        comp = [n % 3 == 0 for n in range(len(ids))]
        frames = iter(_device_frames(gpu_ctx, [t for t, c in zip(texts, comp) if c]))
        datas = [next(frames) if c else t for t, c in zip(texts, comp)]
        specs = [(1, np.frombuffer(i, np.uint8), bytes(rng.integers(0, 256, 16, dtype=np.uint8)),
                  len(t) if c else 0) for i, t, c in zip(ids, texts, comp)]
        third = (len(ids) + 2) // 3
        groups = [(a, min(third, len(ids) - a)) for a in range(0, len(ids), third)]
        files, _, _, _, _ = _build(KEY, datas, specs, groups,
                                   [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in groups])
        self.key = Key(KEY)
        self.packs, self.tree_packs = {}, []
        for pack in files:
            hlen = int.from_bytes(pack[-4:], "little")
            ip = IndexPack(hashlib.sha256(pack).digest())
            for e in parse_header(self.key.decrypt_data(pack[-4 - hlen:-4])):
                ip.add(e.id, e.type, e.offset, e.length, e.uncompressed_len or None)
            self.packs[ip.id] = pack
            self.tree_packs.append(ip)
        self.data_packs = []
        dids = data_ids(r)
        for p in range(0, len(dids), 7):
            ip = IndexPack(bid(f"datapack{p}"))
            for n, i in enumerate(dids[p:p + 7]):
                ip.add(i, 0, 100 * n, 68 + n, 200 if n % 2 else None)
            self.data_packs.append(ip)

    def index_packs(self, without=()):
        from rustic_core_amd.index import IndexPack
        return [IndexPack(p.id, [b for b in p.blobs if b.id not in without])
                for p in self.tree_packs + self.data_packs]

    def index(self, without=()):
        from rustic_core_amd import DeviceIndex
        from rustic_core_amd.index import IndexFile
        return DeviceIndex.from_index_files([IndexFile(self.index_packs(without))])

    def host_index(self, without=()):
        from rustic_core_amd.check import HostIndex
        return HostIndex(self.index_packs(without))

    def reader(self):
        from rustic_core_amd.restore import from_packs
        return from_packs(self.packs)
