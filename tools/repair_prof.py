"""repair.plan_repair on the device beside the same rule in plain Python and
beside check.check_trees (``node_facts="device"``) on the same repository, in
one process, in turns.

The repository is tools/check_trees_prof.py's: 2^12 trees of 64 file nodes
under dir trees of 256 (4113 trees, 262 144 file nodes), every blob sealed on
the device into one pack that read_partial serves from HBM, the content ids in
a data index of packs of 4096 blobs -- clean, and with every 1000th content
id left out, so that one node in a thousand lacks its blob.  The host route
reads the same pack from a host copy.

Times are time.perf_counter around the call and a device synchronise, the
median, min and max of --reps after --warmup unmeasured calls of each route,
the routes taking turns.  The kernel lines are device times of one more call
of the device route under torch.profiler.
"""
import hashlib
import json
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tools")
import check_trees_prof as cp  # noqa: E402  (reads --reps, --warmup and the repository's options)
from rustic_core_amd.check import HostIndex, check_trees  # noqa: E402
from rustic_core_amd.crypto import Key, sealed_layout  # noqa: E402
from rustic_core_amd.index import IndexPack  # noqa: E402
from rustic_core_amd.repair import plan_repair, spread_rounds_per_launch  # noqa: E402

args, say, tp = cp.args, cp.say, cp.tp


def host_index(blobs, pid, content, skip) -> HostIndex:
    """tree_prof.sealed_repo's tree pack and check_trees_prof.with_data's data
    packs as a HostIndex."""
    lens = np.array([len(b) for _, b in blobs], np.int64)
    offs, _ = sealed_layout(lens)
    trees = IndexPack(pid)
    for (i, _), o, n in zip(blobs, offs, lens):
        trees.add(i, 1, int(o), int(n) + 32, None)
    packs = [trees]
    for p in range(0, len(content), cp.PACK_BLOBS):
        ip = IndexPack(bytes([p // cp.PACK_BLOBS % 256, p // cp.PACK_BLOBS // 256]) + bytes(30))
        for n, i in enumerate(content[p:p + cp.PACK_BLOBS]):
            if not (skip and (p + n) % skip == skip - 1):
                ip.add(i.tobytes(), 0, 100 * n, 90, None)
        packs.append(ip)
    return HostIndex(packs)


def kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total,
                 e.count) for e in prof.key_averages()]
    except Exception as e:  # the profiler is a convenience, the clocks above are the result
        say(f"  (no kernel times: {e})")
        return
    for k, t, c in sorted((r for r in rows if "rcdc_rp_" in r[0]), key=lambda r: -r[1]):
        say(f"  {k.split('(')[0]:34s} {t / 1e3:9.3f} ms in {c} launches")
    for label, pat in (("all rcdc_rp_* kernels", ("rcdc_rp_",)),
                       ("rcdc_tr_* kernels (the parse)", ("rcdc_tr_",))):
        say(f"  {label:34s} {sum(t for k, t, _ in rows if any(p in k for p in pat)) / 1e3:9.3f} ms")
    say(f"  {'everything on the device':34s} {sum(t for _, t, _ in rows) / 1e3:9.3f} ms")


def main():
    assert torch.cuda.is_available(), "repair_prof needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}, the routes "
        f"in turns in one process; {spread_rounds_per_launch()} spread rounds per launch")
    key = Key(bytes(range(64)))
    blobs, root, content, total = cp.repository(key, np.random.default_rng(16))
    snap = json.dumps({"time": "2024-01-01T00:00:00+00:00", "tree": root.hex(), "paths": ["/data"],
                       "hostname": "h", "username": "u", "uid": 0, "gid": 0, "tags": []},
                      separators=(",", ":")).encode()
    sealed = key.encrypt_data(snap, bytes(16))
    snaps = [(hashlib.sha256(sealed).digest(), sealed)]
    for name, skip in (("clean", 0), ("1 node in 1000 lacks its blob", 1000)):
        pack, dx, pid = tp.sealed_repo(key, blobs)
        cp.with_data(dx, content, skip)
        hx = host_index(blobs, pid, content, skip)
        host_pack = pack.cpu().numpy().tobytes()
        out = {}

        def read_partial(pack_id, offset, length, pack=pack):
            return pack[offset:offset + length]

        def read_host(pack_id, offset, length, data=host_pack):
            return data[offset:offset + length]

        def device():
            out["device"] = plan_repair(key, dx, snaps, read_partial, device=0)

        def host():
            out["host"] = plan_repair(key, hx, snaps, read_host, device=None)

        def check():
            out["check"] = check_trees(key, dx, [root], read_partial, node_facts="device")
        dev, hst, chk = cp.turns([device, host, check], args.reps, args.warmup)
        assert out["device"].fields() == out["host"].fields()
        plan = out["device"]
        say(f"--- {name}: {len(blobs)} trees, {total / 1e6:.1f} MB of tree text, {len(content)} file "
            f"nodes; {len(plan.changed)} trees change, {len(plan.new_trees)} to save, "
            f"{len(out['check'][0])} findings of check_trees")
        for label, t in (("plan_repair(device=0)", dev), ("plan_repair(device=None)", hst),
                         ('check_trees(node_facts="device")', chk)):
            say(f"{label:34s} median {t[0] * 1e3:9.2f} ms  (min {t[1] * 1e3:.2f}, max {t[2] * 1e3:.2f})")
        s = plan.stats
        say(f"device route: {s['spread_rounds']} spread rounds, {s['text_bytes_to_host']} B of text to "
            f"the host, {s['host_parsed_blobs']} blobs parsed there; host / device = "
            f"{hst[0] / dev[0]:.1f}, device / check_trees = {dev[0] / chk[0]:.2f}")
        kernels(device)
        dx.close()


if __name__ == "__main__":
    main()
