"""Tree blobs on the device: tree.parse_trees (rcdc_tree_parse) in GiB/s of
tree text and per kernel, and tree.find_used_blobs end to end, beside the host
rule tree.parse_tree_host on one thread over the same text.

Two synthetic shapes, as Tree::serialize writes them:
- many: 2^--log2-trees trees (default 16) of --nodes file nodes (default 64)
  with full metadata and one content id each;
- one: one tree whose single file node holds 2^--log2-ids content ids
  (default 20), about 70 MB.
For find_used_blobs each shape is a repository: a root tree of dir nodes over
trees of dir nodes (--fanout each) over the trees of the shape, every blob
sealed on the device and stored, all in one pack that read_partial serves from
HBM; the index is a DeviceIndex.

Times are time.perf_counter around the call and a device synchronise, the
median, min and max of --reps after --warmup unmeasured calls.  The kernel
lines are device times of one more call under torch.profiler (kernels named
rcdc_tr_*); the host baseline runs --host-reps times over --host-trees trees
of the many shape (it is the same work per tree) and once over the one shape.
"""
import argparse
import hashlib
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rustic_core_amd import DeviceIndex  # noqa: E402
from rustic_core_amd.crypto import Key, _ctx, make_refs, sealed_layout  # noqa: E402
from rustic_core_amd.index import IndexFile, IndexPack  # noqa: E402
from rustic_core_amd.tree import find_used_blobs, parse_tree_host, parse_trees  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-trees", type=int, default=16)
ap.add_argument("--nodes", type=int, default=64)
ap.add_argument("--log2-ids", type=int, default=20)
ap.add_argument("--fanout", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--host-trees", type=int, default=256)
ap.add_argument("--no-e2e", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
HEXD = np.frombuffer(b"0123456789abcdef", np.uint8)
TIME = b"2024-05-06T07:08:09.123456789+02:00"


def say(*a):
    print(*a, flush=True)


def hexed(ids: np.ndarray) -> np.ndarray:
    out = np.empty(ids.shape[:-1] + (ids.shape[-1] * 2,), np.uint8)
    out[..., 0::2] = HEXD[ids >> 4]
    out[..., 1::2] = HEXD[ids & 15]
    return out


def digits(v: np.ndarray, width: int) -> np.ndarray:
    out = np.empty(v.shape + (width,), np.uint8)
    for k in range(width):
        out[..., width - 1 - k] = 0x30 + (v // 10 ** k) % 10
    return out


def rows_of(parts, cols, n):
    it = iter(cols)
    return np.concatenate([np.broadcast_to(np.frombuffer(p, np.uint8), (n, len(p))) if p is not None
                           else next(it) for p in parts], axis=1)


def _meta(mode: bytes):
    return (b'","mode":' + mode + b',"mtime":"' + TIME + b'","atime":"' + TIME + b'","ctime":"' +
            TIME + b'","uid":1000,"gid":1000,"user":"alice","group":"users","inode":')


def file_trees(rng, n_trees: int, nodes: int):
    """n_trees texts of ``nodes`` file nodes, every number of a fixed width,
    so all trees have one length; returns an (n_trees, length) byte matrix."""
    n = n_trees * nodes
    parts = [b'{"name":"f', None, b'","type":"file' + _meta(b"33188"), None,
             b',"device_id":64769,"size":', None, b',"links":1,"content":["', None, b'"]},']
    cols = [digits(np.arange(n) % 10 ** 8, 8), digits(rng.integers(10 ** 7, 10 ** 8, n), 8),
            digits(rng.integers(10 ** 6, 10 ** 7, n), 7),
            hexed(rng.integers(0, 256, (n, 32), dtype=np.uint8))]
    body = rows_of(parts, cols, n).reshape(n_trees, -1)[:, :-1]
    return np.concatenate([np.broadcast_to(np.frombuffer(b'{"nodes":[', np.uint8), (n_trees, 10)),
                           body, np.broadcast_to(np.frombuffer(b"]}\n", np.uint8), (n_trees, 3))],
                          axis=1)


def dir_tree(ids) -> bytes:
    """One tree of dir nodes over ``ids`` ((k, 32) uint8)."""
    k = len(ids)
    parts = [b'{"name":"d', None, b'","type":"dir' + _meta(b"2147484141"), None,
             b',"device_id":64769,"links":2,"content":null,"subtree":"', None, b'"},']
    cols = [digits(np.arange(k), 8), digits(np.arange(k) + 10 ** 7, 8), hexed(ids)]
    return b'{"nodes":[' + rows_of(parts, cols, k).reshape(-1)[:-1].tobytes() + b"]}\n"


def one_tree(rng, n_ids: int) -> bytes:
    ids = hexed(rng.integers(0, 256, (n_ids, 32), dtype=np.uint8))
    body = rows_of([b'"', None, b'",'], [ids], n_ids).reshape(-1)[:-1].tobytes()
    return (b'{"nodes":[{"name":"big","type":"file' + _meta(b"33188") +
            b'12345678,"device_id":64769,"size":1099511627776,"links":1,"content":[' + body +
            b"]}]}\n")


def clocked(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def line(name, t, nbytes, extra=""):
    med, lo, hi = t
    say(f"{name:34s} median {med * 1e3:10.2f} ms  (min {lo * 1e3:.2f}, max {hi * 1e3:.2f})  "
        f"{nbytes / med / 2 ** 30:8.3f} GiB/s of tree text{extra}")


def kernels(fn):
    """Device time per rcdc_tr_* kernel of one call of fn."""
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total)
                for e in prof.key_averages() if "rcdc_tr_" in e.key]
    except Exception as e:  # the profiler is a convenience, the clocks above are the result
        say(f"  (no kernel times: {e})")
        return
    if not rows:
        say("  (the profiler saw no rcdc_tr_* kernel)")
        return
    total = sum(t for _, t in rows)
    for k, t in sorted(rows, key=lambda r: -r[1]):
        say(f"  {k.split('(')[0]:34s} {t / 1e3:9.3f} ms  {100 * t / total:5.1f} %")
    say(f"  {'all rcdc_tr_* kernels':34s} {total / 1e3:9.3f} ms")


def sealed_repo(key, blobs):
    """``blobs``: [(id, text bytes or a row of a byte matrix)].  All sealed on
    the device into one arena that stands for one pack; returns (device
    arena, DeviceIndex, pack id)."""
    lens = np.array([len(b) for _, b in blobs], np.int64)
    in_offs = np.concatenate([[0], np.cumsum((lens + 15) // 16 * 16)[:-1]]).astype(np.uint64)
    host = np.zeros(int(in_offs[-1]) + int(lens[-1]) + 64, np.uint8)
    for o, (_, b) in zip(in_offs, blobs):
        host[int(o):int(o) + len(b)] = np.frombuffer(b, np.uint8) if isinstance(b, bytes) else b
    out_offs, total = sealed_layout(lens)
    d_in = torch.from_numpy(host).to(dev)
    d_out = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    nonces = np.random.default_rng(1).integers(0, 256, (len(blobs), 16), dtype=np.uint8)
    key.seal_blobs(d_in.data_ptr(), make_refs(in_offs, lens, out_offs, nonces), d_out.data_ptr(),
                   torch.cuda.current_stream(dev).cuda_stream, _ctx(0))
    torch.cuda.synchronize()
    pid = hashlib.sha256(b"tree_prof pack").digest()
    ip = IndexPack(pid)
    for (i, _), o, n in zip(blobs, out_offs, lens):
        ip.add(i, 1, int(o), int(n) + 32, None)
    return d_out, DeviceIndex.from_index_files([IndexFile([ip])]), pid


def e2e(key, name, leaves, total_text):
    """find_used_blobs over a root, dir trees of --fanout and ``leaves``."""
    blobs = list(leaves)
    level = np.frombuffer(b"".join(i for i, _ in leaves), np.uint8).reshape(-1, 32)
    while True:
        texts = [dir_tree(level[a:a + args.fanout]) for a in range(0, len(level), args.fanout)]
        ids = [hashlib.sha256(t).digest() for t in texts]
        blobs += list(zip(ids, texts))
        total_text += sum(len(t) for t in texts)
        if len(texts) == 1:
            break
        level = np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32)
    pack, dx, pid = sealed_repo(key, blobs)

    def read_partial(pack_id, offset, length):
        return pack[offset:offset + length]
    out = {}

    def run():
        out["used"] = find_used_blobs(key, dx, [ids[0]], read_partial)
    t = clocked(run, args.reps, args.warmup)
    line(f"{name}: find_used_blobs, {len(blobs)} trees", t, total_text,
         f"  {int(out['used'].shape[0])} used ids")
    dx.close()


def shape(key, name, texts, ids, host_texts, host_reps):
    """texts: list of bytes or a byte matrix; ids: their tree ids or None."""
    n = len(texts)
    if isinstance(texts, np.ndarray):
        width = texts.shape[1]
        stride = (width + 15) // 16 * 16
        host = np.zeros((n, stride), np.uint8)
        host[:, :width] = texts
        offs, lens = (np.arange(n) * stride).tolist(), [width] * n
        total = n * width
        host = host.reshape(-1)
    else:
        offs, lens, total = [0], [len(texts[0])], len(texts[0])
        host = np.frombuffer(texts[0] + b"\0" * 16, np.uint8).copy()
    d = torch.from_numpy(host).to(dev)
    res = parse_trees(d, offs, lens)
    assert int(res.blobs["status"].sum()) == 0, "a synthetic tree is outside G_T"
    say(f"--- {name}: {n} trees, {total / 1e6:.1f} MB of tree text, {res.nodes} nodes, "
        f"{res.n_data_ids} content ids")
    del res
    line("parse_trees (text in HBM)", clocked(lambda: parse_trees(d, offs, lens), args.reps,
                                              args.warmup), total)
    kernels(lambda: parse_trees(d, offs, lens))
    hb = sum(len(t) for t in host_texts)
    t = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        for x in host_texts:
            parse_tree_host(x)
        t.append(time.perf_counter() - t0)
    line(f"parse_tree_host, 1 thread, {len(host_texts)} trees", (statistics.median(t), min(t), max(t)),
         hb)
    del d
    if not args.no_e2e:
        e2e(key, name, [(i, t) for i, t in zip(ids, texts)], total)


def main():
    assert torch.cuda.is_available(), "tree_prof needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}; the "
        "baseline is parse_tree_host (json.loads) on one thread: the reference's serde_json on "
        "MAX_TREE_LOADER = 4 threads cannot be run here")
    key = Key(bytes(range(64)))
    rng = np.random.default_rng(16)
    many = file_trees(rng, 1 << args.log2_trees, args.nodes)
    ids = [hashlib.sha256(r).digest() for r in many] if not args.no_e2e else [b""] * len(many)
    shape(key, f"many (2^{args.log2_trees} x {args.nodes} nodes)", many, ids,
          [r.tobytes() for r in many[:args.host_trees]], args.host_reps)
    del many
    one = one_tree(rng, 1 << args.log2_ids)
    shape(key, f"one (1 node, 2^{args.log2_ids} ids)", [one], [hashlib.sha256(one).digest()], [one], 1)


if __name__ == "__main__":
    main()
