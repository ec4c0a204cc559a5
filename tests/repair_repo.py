"""Small repositories for the repair tests, over tests/used_blobs_repo.py's
builder: one tree per rule of ``repair snapshots`` under a first snapshot, the
tree reached at level 1 and again at level 3 under a second, a clean third, a
tree that hangs under a symlink under a fourth, a tree with a key ``Node``
does not know under a fifth, and (on request) a file without content under a
sixth.  Also the repository as plain host objects -- an identity key, one
pack of tree texts, a dict index -- for ``plan_repair(device=None)``.

The data index is tests/check_trees_repo.py's: every content id of a file
node but the all-zero id and MISSING, in packs of 7, so a device test can pack
the same repository with ``check_trees_repo.Packed``.
"""
import hashlib
import json

from tests import used_blobs_repo as ubr
from tests.check_trees_repo import MISSING, NULL, data_ids
from tests.tree_json_cases import TIME, serialize

EMPTY = b'{"nodes":[]}\n'
EMPTY_ID = hashlib.sha256(EMPTY).digest()


def meta(n: int, size: int = 0) -> dict:
    m = {"mode": 33188, "mtime": TIME, "atime": TIME, "ctime": TIME, "uid": 1000, "gid": 100,
         "user": "alice", "group": "users", "inode": 2000 + n, "device_id": 64769}
    if size:
        m["size"] = size
    m["links"] = 1
    return m


def f(name, ids, size=0, n=0) -> dict:
    """A file node in serde's order; ``ids``: names of data blobs, or ids."""
    return dict({"name": name, "type": "file"}, **meta(n, size),
                content=[i.hex() if isinstance(i, bytes) else ubr.did(i).hex() for i in ids])


def d(name, tid, n=0) -> dict:
    o = dict({"name": name, "type": "dir"}, **meta(n), content=None)
    if tid is not None:
        o["subtree"] = tid.hex()
    return o


def build(no_content: bool = False) -> ubr.Repo:
    r = ubr.Repo()
    # -- the rules, one tree each
    nosub = r.add("nosub", [d("hollow", None), f("ok", ["a.0"], n=1)])
    zero = r.add("zero", [f("z", ["a.1", NULL], n=2)])
    fifo = r.add("fifo", [{"name": "pipe", "type": "fifo", "content": [ubr.did(MISSING[1]).hex()]},
                          f("ok", ["a.2"], n=3)])
    hidden = r.add("hidden", [f("h", [MISSING[0]], n=4)])
    nondir = r.add("nondir", [dict({"name": "ln", "type": "symlink", "linktarget": "t"},
                                   content=None, subtree=hidden.hex())])
    # its only subtree is the empty tree, which no pack holds: lost, processed as the
    # empty tree, and the empty tree is what it was
    sameid = r.add("sameid", [d("void", EMPTY_ID)])
    twin1 = r.add("twin1", [f("x", ["a.3", MISSING[0]], 9, n=5)])
    twin2 = r.add("twin2", [f("x", ["a.3", MISSING[1]], 9, n=5)])
    already = r.add("already", [f("y", [MISSING[0]], 4, n=6)])
    r.add("already-repaired", [f("y.repaired", [], n=6)])  # in the index, under no node
    sizefix = r.add("sizefix", [f("wrong", ["a.4", "a.5"], 7, n=7), f("cut", ["a.6", MISSING[1]], 8, n=8)])
    sizeonly = r.add("sizeonly", [f("wrong", ["a.4", "a.5"], 7, n=7)])
    lost = r.add("lostleaf", [f("never", ["a.7"], n=9)])  # an index ``without`` it lacks it
    keeps = r.add("keeps", [d("gone", lost), f("stays", ["a.8"], n=10)])
    rules = r.add("rules", [d("nosub", nosub), d("zero", zero), d("fifo", fifo), d("sameid", sameid),
                            d("twin1", twin1), d("twin2", twin2), d("already", already),
                            d("sizefix", sizefix), d("sizeonly", sizeonly), d("keeps", keeps)])
    # -- P is first reached at level 1 and hangs again under R at level 3; the damage is below P
    leaf = r.add("backleaf", [f("b", ["a.9", MISSING[0]], 3, n=11)])
    p = r.add("P", [d("leafd", leaf)])
    rr = r.add("R", [d("back", p)])
    q = r.add("Q", [d("r", rr)])
    back = r.add("backroot", [d("p", p), d("q", q)])
    clean = r.add("cleanroot", [d("fifo", fifo), d("sizeonly", sizeonly), f("top", ["a.0", "a.1"], n=12)])
    # check_trees follows the symlink's subtree and repair does not: a snapshot of its own
    odd = r.add("oddroot", [d("nondir", nondir)])
    # a tree outside the device's grammar (an unknown key) with damage in it and below it
    below = r.add("hostbelow", [f("hb", ["a.11", MISSING[1]], 5, n=14)])
    host = r.add("host", [f("hf", ["a.10", MISSING[0]], 6, n=15), d("below", below)],
                 extra="generic_attributes")
    r.snapshots = [rules, back, clean, odd, r.add("hostroot", [d("host", host)])]
    if no_content:
        nc = r.add("nc", [f("fine", ["a.0"], n=13), {"name": "nc", "type": "file"}])
        r.snapshots.append(r.add("ncroot", [d("a", r.add("ncmid", [d('b"q', nc)]))]))
    return r


def snapshot_file(tree: bytes, n: int = 0, **kw) -> bytes:
    """A snapshot file's JSON (the ``sealed`` bytes under the identity key)."""
    o = {"time": TIME, "program_version": "rustic 0.9", "tree": tree.hex(),
         "paths": ["/home"], "hostname": f"host{n}", "username": "alice", "uid": 1000, "gid": 100,
         "tags": ["daily"]}
    o.update(kw)
    return json.dumps(o, separators=(",", ":")).encode()


class PlainKey:
    def decrypt_data(self, data: bytes) -> bytes:
        return bytes(data)


class HostRepo:
    """``repo`` behind ``plan_repair(device=None)``: ``index`` is a dict
    {id: (pack id, IndexBlob)}; the trees in ``without`` are in no pack."""
    PACK = b"T" * 32

    def __init__(self, repo: ubr.Repo, without=()):
        from rustic_core_amd.index import IndexBlob
        from tests.prune_cases import bid
        self.repo, self.key = repo, PlainKey()
        self.names = {v: k for k, v in repo.names.items()}
        self.index, self.pack = {}, b""
        for tid, text in repo.trees.items():
            if tid not in without:
                self.index[tid] = (self.PACK, IndexBlob(tid, 1, len(self.pack), len(text), None))
                self.pack += text
        dids = data_ids(repo)
        for p in range(0, len(dids), 7):  # check_trees_repo.Packed's data packs
            for n, i in enumerate(dids[p:p + 7]):
                self.index[i] = (bid(f"datapack{p}"),
                                 IndexBlob(i, 0, 100 * n, 68 + n, 200 if n % 2 else None))
        self.snapshots = []
        for n, t in enumerate(repo.snapshots):
            sealed = snapshot_file(t, n)
            self.snapshots.append((hashlib.sha256(sealed).digest(), sealed))

    def read_partial(self, pack_id, offset, length):
        assert bytes(pack_id) == self.PACK
        return self.pack[offset:offset + length]

    def length(self, name) -> int:
        """data_length of the data blob ``name``."""
        b = self.index[ubr.did(name)][1]
        return b.uncompressed_length or b.length - 32

    def plan(self, opts=None, snapshots=None):
        from rustic_core_amd.repair import RepairSnapshotsOptions, plan_repair
        return plan_repair(self.key, self.index, self.snapshots if snapshots is None else snapshots,
                           self.read_partial, opts or RepairSnapshotsOptions(), device=None)


def tree_text(nodes) -> bytes:
    return serialize({"nodes": nodes})


def tid(text: bytes) -> bytes:
    return hashlib.sha256(text).digest()
