"""The reference's eight check repositories (tests/golden/check_fixtures.json,
made by make_check_golden.py) opened for check.check_repository, and its
recorded CheckResults in the shape this project's findings take.  Shared by
tests/test_check_host.py and tests/test_gpu_check.py."""
import base64
import json
import os

from tests.test_crypto_oracle import _kdf, _master

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "check_fixtures.json")))
N_M = json.load(open(os.path.join(HERE, "golden", "check_n_m.json")))
REPOS = sorted(FIX["repos"])
# the one snapshot of a test the reference has switched off (its #[case] is commented out)
INACTIVE = "repo-index-missing-blob.tar.gz"
TYPES = {"Data": 0, "Tree": 1}


class Repo:
    """A fixture's files behind the callables of check_repository."""

    def __init__(self, name: str, oracle_mod):
        self.files = {k: base64.b64decode(v) for k, v in FIX["repos"][name]["files"].items()}
        kf = json.loads([v for k, v in self.files.items() if k.startswith("repo/keys/")][0])
        mk = json.loads(oracle_mod.open_(_kdf(kf, FIX["password"]), base64.b64decode(kf["data"])))
        self.master = _master(mk)
        self.by_type = {"index": {}, "pack": {}, "snapshot": {}}
        for k, v in self.files.items():
            for prefix, t in (("repo/index/", "index"), ("repo/data/", "pack"),
                              ("repo/snapshots/", "snapshot")):
                if k.startswith(prefix):
                    self.by_type[t][bytes.fromhex(k.rsplit("/", 1)[1])] = v

    def list_with_size(self, file_type):
        return [(i, len(v)) for i, v in self.by_type[file_type].items()]

    def read_full(self, file_type, id_):
        return self.by_type[file_type][bytes(id_)]

    def read_partial(self, pack_id, offset, length):
        return self.by_type["pack"][bytes(pack_id)][offset:offset + length]

    def snapshots(self):
        return [self.by_type["snapshot"][i] for i in sorted(self.by_type["snapshot"])]


def recorded(name: str):
    """The recorded findings as (level, kind, fields) with ids as bytes and
    blob types as 0 / 1; of an ErrorCheckingTrees the source's kind and the
    short tree id."""
    out = []
    for r in FIX["repos"][name]["results"]:
        f = {}
        for k, v in r["fields"].items():
            if k in ("id", "blob_id"):
                v = bytes.fromhex(v)
            elif k in ("blob_type", "expected") and v in TYPES:
                v = TYPES[v]
            elif k == "source":
                assert v["guidance"] == "Tree ID `{tree_id}` not found in index"
                v = (v["kind"], dict(v["context"])["tree_id"])
            f[k] = v
        out.append((r["level"], r["kind"], f))
    return out


def normal(results):
    """check_repository's results in ``recorded``'s shape."""
    out = []
    for level, finding in results:
        f = dict(finding.fields)
        if finding.kind == "ErrorCheckingTrees":
            e = f["source"]
            text = str(e)
            assert "Tree ID `" in text and "` not found in index" in text
            f["source"] = (e.kind.name, text.split("Tree ID `", 1)[1][:8])
        out.append((level, finding.kind, f))
    return out


def run(name: str, oracle_mod, key, device, snapshot_trees_device=None):
    from oracle import zstd_ref as zr
    from rustic_core_amd.check import check_repository
    from rustic_core_amd.tree import snapshot_trees
    repo = Repo(name, oracle_mod)
    k = key(repo.master)
    trees = snapshot_trees(k, repo.snapshots(), device=snapshot_trees_device, decode=zr.decompress)
    return check_repository(k, repo.list_with_size, repo.read_full, repo.read_partial, trees,
                            read_data=True, device=device, decode=zr.decompress)
