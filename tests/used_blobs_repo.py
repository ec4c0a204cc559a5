"""A small repository of trees for the find_used_blobs tests, as plain
objects: 3 snapshots over 40 trees, 4 levels deep, with shared subtrees, a
tree reached twice in one level, a tree the device's grammar leaves to the
host (an unknown key) that has children of its own, and a tree that is only
reached through the subtree of a node that is no dir.  Also the walk of
tree.find_used_blobs written down once more, over the objects.
"""
import hashlib
import json

from tests.tree_json_cases import meta, serialize


def did(name: str) -> bytes:
    """The id of a data blob that exists only by name."""
    return hashlib.sha256(b"data:" + name.encode()).digest()


class Repo:
    def __init__(self):
        self.trees = {}      # tree id -> text, in the order built (leaves first)
        self.names = {}      # tree id -> name
        self.snapshots = []  # root tree ids

    def add(self, name, nodes, extra=None) -> bytes:
        o = {"nodes": nodes}
        text = serialize(o)
        if extra:  # a key Node does not know, after "name": outside G_T, fine for serde
            text = text.replace(b'"type":', b'"' + extra.encode() + b'":{"a":[1,2]},"type":', 1)
        tid = hashlib.sha256(text).digest()
        assert tid not in self.trees, name
        self.trees[tid] = text
        self.names[tid] = name
        return tid


def _file(name, ids):
    return dict({"name": name, "type": "file"}, **meta(len(ids)), content=[did(i).hex() for i in ids])


def _dir(name, tid):
    return dict({"name": name, "type": "dir"}, **meta(0), content=None, subtree=tid.hex())


def build() -> Repo:
    r = Repo()
    # level 3: 18 leaves; neighbours share a data blob, leaf 5 is empty
    leaves = [r.add(f"leaf{i}", [] if i == 5 else
                    [_file(f"a{i}", [f"l{i}.0", f"l{i}.1", f"l{i + 1}.0"]), _file("same", ["shared"]),
                     _file("empty", [])]) for i in range(18)]
    # only reached through a symlink node's subtree: followed, never inserted
    hidden = r.add("hidden", [_file("h", ["hidden.0", "shared"])])
    # level 2: 12 trees, two leaves each, every leaf but the first and last shared
    mids = []
    for j in range(12):
        nodes = [_dir("x", leaves[(3 * j) // 2]), _file(f"m{j}", [f"m{j}.0"]),
                 _dir("y", leaves[(3 * j) // 2 + 1])]
        if j == 4:
            nodes.append(dict({"name": "ln", "type": "symlink", "linktarget": "t"},
                              subtree=hidden.hex()))
        mids.append(r.add(f"mid{j}", nodes, extra="generic_attributes" if j == 7 else None))
    # level 1: 6 trees over the mids; mid7 (the host's) is under top2 and top3
    tops = [r.add(f"top{k}", [_dir(f"d{m}", mids[m]) for m in (2 * k, 2 * k + 1, (2 * k + 3) % 12)]
                  + [_file("t", [f"t{k}", "shared"])]) for k in range(6)]
    # level 0: 3 snapshot roots; top1 is reached from root0 and root1 in one level, and
    # twice within root0
    r.snapshots = [
        r.add("root0", [_dir("a", tops[0]), _dir("b", tops[1]), _dir("again", tops[1]),
                        _file("r0", ["r0.0"])]),
        r.add("root1", [_dir("b", tops[1]), _dir("c", tops[2]), _dir("d", tops[3])]),
        r.add("root2", [_dir("e", tops[4]), _dir("f", tops[5]), _file("r2", ["r0.0", "r2.0"])]),
    ]
    assert len(r.trees) == 40
    return r


def walk(r: Repo, roots=None):
    """The used ids in find_used_blobs' order, and the trees level by level."""
    roots = list(dict.fromkeys(r.snapshots if roots is None else roots))
    used = list(roots)
    visited = set(roots)
    frontier, levels = list(roots), []
    while frontier:
        levels.append(frontier)
        data, dirs, subtrees = [], [], []
        for tid in frontier:
            for n in json.loads(r.trees[tid])["nodes"]:
                if n["type"] == "file":
                    data += [bytes.fromhex(i) for i in n.get("content") or []]
                if n.get("subtree"):
                    subtrees.append(bytes.fromhex(n["subtree"]))
                    if n["type"] == "dir":
                        dirs.append(subtrees[-1])
        for i in data + dirs:
            if i not in used:
                used.append(i)
        frontier = []
        for i in subtrees:
            if i not in visited:
                visited.add(i)
                frontier.append(i)
    return used, levels
