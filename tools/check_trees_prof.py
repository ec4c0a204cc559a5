"""check.check_trees with the node facts judged on the device
(``node_facts="device"``: rcdc_tree_nodes, rcdc_check_trees_level,
rcdc_tree_names) beside the route that brings every tree blob's text to the
host parser (``node_facts="host"``), in one process, in turns.

The repository is tools/tree_prof.py's "many" kind: 2^--log2-trees trees
(default 12) of --nodes file nodes (default 64) with full metadata and one
content id each, under dir trees of --fanout, every blob sealed on the device
into one pack that read_partial serves from HBM.  The content ids are in a
data index of packs of 4096 blobs.  Two indexes over the same trees:
- clean: every content id is in the data index, nothing is found;
- findings: every 1000th content id is left out, so one node in a thousand
  has a FileBlobNotInIndex.

Times are time.perf_counter around the call and a device synchronise, the
median, min and max of --reps after --warmup unmeasured calls of each route,
the routes taking turns.  "around the batch calls" is the time one call of
the device route spends in tree._level_groups (the frontier's lookup, the
pack reads in Python and read.read_blobs), which both routes share and this
tool leaves as it is.  The kernel lines are device times of one more call of
the device route under torch.profiler.
"""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--log2-trees", type=int, default=12)
ap.add_argument("--nodes", type=int, default=64)
ap.add_argument("--fanout", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
args = ap.parse_args()

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tools")
argv, sys.argv = sys.argv, sys.argv[:1]  # tree_prof reads its own options on import
import tree_prof as tp  # noqa: E402
sys.argv = argv
from rustic_core_amd import tree  # noqa: E402
from rustic_core_amd.check import check_trees  # noqa: E402
from rustic_core_amd.crypto import Key  # noqa: E402
from rustic_core_amd.index import IndexPack  # noqa: E402

say = tp.say
PACK_BLOBS = 4096


def repository(key, rng):
    """(the tree blobs as tree_prof.sealed_repo takes them, the root's id, the
    content ids, the bytes of tree text)."""
    import hashlib
    many = tp.file_trees(rng, 1 << args.log2_trees, args.nodes)
    blobs = [(hashlib.sha256(r).digest(), r) for r in many]
    total = many.size
    level = np.frombuffer(b"".join(i for i, _ in blobs), np.uint8).reshape(-1, 32)
    while True:
        texts = [tp.dir_tree(level[a:a + args.fanout]) for a in range(0, len(level), args.fanout)]
        ids = [hashlib.sha256(t).digest() for t in texts]
        blobs += list(zip(ids, texts))
        total += sum(len(t) for t in texts)
        if len(texts) == 1:
            break
        level = np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32)
    # the content ids, read back out of the text by the device parser
    width = many.shape[1]
    stride = (width + 15) // 16 * 16
    host = np.zeros((len(many), stride), np.uint8)
    host[:, :width] = many
    res = tree.parse_trees(torch.from_numpy(host.reshape(-1)).to(tp.dev),
                           (np.arange(len(many)) * stride).tolist(), [width] * len(many))
    content = res.data_ids.cpu().numpy()
    return blobs, ids[0], content, total


def with_data(dx, content, skip):
    """``dx`` with the content ids in data packs, every ``skip``-th left out (0: none)."""
    packs = []
    for p in range(0, len(content), PACK_BLOBS):
        ip = IndexPack(bytes([p // PACK_BLOBS % 256, p // PACK_BLOBS // 256]) + bytes(30))
        for n, i in enumerate(content[p:p + PACK_BLOBS]):
            if skip and (p + n) % skip == skip - 1:
                continue
            ip.add(i.tobytes(), 0, 100 * n, 90, None)
        packs.append(ip)
    dx.extend(packs)
    return dx


def turns(fns, reps, warmup):
    """The median, min and max of each of ``fns``, called in turns."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[k].append(time.perf_counter() - t0)
    return [(statistics.median(x), min(x), max(x)) for x in t]


def kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total)
                for e in prof.key_averages()]
    except Exception as e:  # the profiler is a convenience, the clocks above are the result
        say(f"  (no kernel times: {e})")
        return
    mine = [(k, t) for k, t in rows if "rcdc_tr_" in k or "rcdc_ct_" in k]
    for k, t in sorted(mine, key=lambda r: -r[1]):
        say(f"  {k.split('(')[0]:34s} {t / 1e3:9.3f} ms")
    say(f"  {'all rcdc_tr_* and rcdc_ct_* kernels':34s} {sum(t for _, t in mine) / 1e3:9.3f} ms")
    say(f"  {'everything else on the device':34s} "
        f"{sum(t for k, t in rows if (k, t) not in mine) / 1e3:9.3f} ms  (open, decode, lookups, copies)")


def shared_part(fn):
    """Seconds of one call of ``fn`` spent inside tree._level_groups."""
    inner, spent = tree._level_groups, [0.0]

    def timed(*a, **kw):
        it = inner(*a, **kw)
        while True:
            t0 = time.perf_counter()
            try:
                item = next(it)
            except StopIteration:
                return
            finally:
                torch.cuda.synchronize()
                spent[0] += time.perf_counter() - t0
            yield item
    tree._level_groups = timed
    try:
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        whole = time.perf_counter() - t0
    finally:
        tree._level_groups = inner
    return spent[0], whole


def main():
    assert torch.cuda.is_available(), "check_trees_prof needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}, the two "
        "routes in turns in one process")
    key = Key(bytes(range(64)))
    rng = np.random.default_rng(16)
    blobs, root, content, total = repository(key, rng)
    n_trees = len(blobs)
    for name, skip in (("clean", 0), ("findings (1 node in 1000)", 1000)):
        pack, dx, _ = tp.sealed_repo(key, blobs)
        with_data(dx, content, skip)
        out = {}

        def read_partial(pack_id, offset, length, pack=pack):
            return pack[offset:offset + length]

        def run(facts):
            stats = {}
            out[facts] = check_trees(key, dx, [root], read_partial, node_facts=facts, stats=stats)
            out[facts + " stats"] = stats
        (dev, host) = turns([lambda: run("device"), lambda: run("host")], args.reps, args.warmup)
        assert out["device"] == out["host"]
        say(f"--- {name}: {n_trees} trees, {total / 1e6:.1f} MB of tree text, "
            f"{len(content)} file nodes, {len(out['device'][0])} findings, "
            f"{len(out['device'][1])} packs referred to")
        for label, t in (('node_facts="device"', dev), ('node_facts="host"', host)):
            s = out[label.split('"')[1] + " stats"]
            say(f"{label:22s} median {t[0] * 1e3:9.2f} ms  (min {t[1] * 1e3:.2f}, max {t[2] * 1e3:.2f})"
                f"  to the host: {s['text_bytes_to_host']} B of text, {s['name_bytes_to_host']} B of "
                f"names, {s['host_parsed_blobs']} blobs parsed there")
        say(f"host / device = {host[0] / dev[0]:.2f}; spread of the repeats: device "
            f"{(dev[2] - dev[1]) * 1e3:.2f} ms, host {(host[2] - host[1]) * 1e3:.2f} ms")
        spent, whole = shared_part(lambda: run("device"))
        say(f"around the batch calls (tree._level_groups: lookup, pack reads, read_blobs): "
            f"{spent * 1e3:.2f} of {whole * 1e3:.2f} ms of a device-route call")
        kernels(lambda: run("device"))
        dx.close()


if __name__ == "__main__":
    main()
