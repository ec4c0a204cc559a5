"""check on the device, measured: the index pass (rcdc_check_packs) and
check_pack_batch beside the loop over read.check_pack.  Writes
profiles/check_prof.txt (--out).

1. The index pass at --log2 entries (default 20,24) in packs of --pack-blobs
   (500, as tools/index_load_prof.py): every pack in order, and 1 % of the
   packs shuffled; beside it a device copy of the same 48 bytes per entry
   (ids and locs cloned) and, at 2^20, the Python rule (check.index_pass_host
   over IndexPacks); then 2^20 entries in packs of --small-pack-blobs (16),
   where a workgroup per pack has little to do.  The two device sides and the copy are interleaved in one
   process: a warm-up round, then the median of --reps rounds,
   time.perf_counter around the call and a device synchronise.
2. check_pack_batch against the loop over read.check_pack on the same
   --packs (256) device-built packs of about 1 MiB (16 blobs of 64 KiB, every
   second one a zstd frame made on the device), interleaved the same way,
   then the batch's stage times by events from one more run.
"""
import argparse
import hashlib
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rustic_core_amd import check  # noqa: E402
from rustic_core_amd.crypto import Key, _ctx  # noqa: E402
from rustic_core_amd.index import IndexPack  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", default="20,24")
ap.add_argument("--pack-blobs", type=int, default=500)
ap.add_argument("--small-pack-blobs", type=int, default=16)
ap.add_argument("--packs", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=__file__.rsplit("/tools/", 1)[0] + "/profiles/check_prof.txt")
args = ap.parse_args()
dev = torch.device("cuda:0")
LINES = []


def say(*a):
    line = " ".join(str(x) for x in a)
    LINES.append(line)
    print(line, flush=True)


def interleaved(sides: dict, reps: int) -> dict:
    """{name: median seconds}: a warm-up round, then ``reps`` rounds in which
    every side runs once, one after the other."""
    times = {k: [] for k in sides}
    for r in range(reps + 1):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                times[name].append(time.perf_counter() - t0)
    return {k: statistics.median(v) for k, v in times.items()}


def entries(rng, n: int, per_pack: int):
    """ids, locs (pack, offset, length, uncompressed length) and ranges of
    n entries in packs written back to back."""
    ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    lens = rng.integers(100, 100_000, n, dtype=np.int64)
    packs = n // per_pack
    offs = (np.cumsum(lens.reshape(packs, per_pack), 1) - lens.reshape(packs, per_pack)).reshape(-1)
    ulens = np.where(rng.random(n) < 0.5, lens * 3, 0)
    locs = np.stack([np.repeat(np.arange(packs), per_pack), offs, lens, ulens], 1).astype(np.uint32)
    ranges = np.zeros(packs, check.CK_RANGE)
    ranges["first"], ranges["count"] = np.arange(packs) * per_pack, per_pack
    return ids, locs, ranges


def index_pass(lg: int, per: int, python_rule: bool):
    rng = np.random.default_rng(lg)
    n = 1 << lg
    n -= n % per
    ids, locs, ranges = entries(rng, n, per)
    mixed = locs.copy()
    mixed_ids = ids.copy()
    shuffled = rng.choice(len(ranges), max(len(ranges) // 100, 1), replace=False)
    for p in shuffled:
        perm = rng.permutation(per) + p * per
        mixed[p * per:(p + 1) * per] = locs[perm]
        mixed_ids[p * per:(p + 1) * per] = ids[perm]
    up = lambda a: torch.from_numpy(a).to(dev)
    d_ids, d_locs = up(ids), up(locs.view(np.int32))
    m_ids, m_locs = up(mixed_ids), up(mixed.view(np.int32))
    types = torch.zeros(n, dtype=torch.uint8, device=dev)
    got = {}

    def run(i, l, key):
        def fn():
            got[key] = check.run_check_packs(i, l[:, 1], l[:, 2], l[:, 3], types, ranges)
        return fn
    t = interleaved({"in order": run(d_ids, d_locs, "a"), "1% shuffled": run(m_ids, m_locs, "b"),
                     "copy 48 B/entry": lambda: (d_ids.clone(), d_locs.clone())}, args.reps)
    assert got["a"].total == 0 and got["a"].packs_sorted_on_device == 0
    assert got["b"].total == 0 and got["b"].packs_sorted_on_device == len(shuffled)
    say(f"index pass, 2^{lg} = {n} entries in {len(ranges)} packs of {per}:")
    copy = n / t["copy 48 B/entry"]
    for name, s in t.items():
        say(f"  {name:<18} {s * 1e3:9.3f} ms  {n / s / 1e6:10.1f} M entries/s"
            f"  {100 * (n / s) / copy:6.1f} % of the copy's rate")
    if python_rule:
        packs = []
        for r in ranges:
            f, c = int(r["first"]), int(r["count"])
            ip = IndexPack(bytes(32))
            for e in range(f, f + c):
                ip.add(b"", 0, int(locs[e, 1]), int(locs[e, 2]), int(locs[e, 3]) or None)
            packs.append(ip)
        t0 = time.perf_counter()
        found = sum(len(check.index_pass_host(p)) for p in packs)
        s = time.perf_counter() - t0
        assert found == 0
        say(f"  {'python rule':<18} {s * 1e3:9.3f} ms  {n / s / 1e6:10.1f} M entries/s"
            f"  {100 * (n / s) / copy:6.1f} % of the copy's rate   (one run)")


def build_packs(n_packs: int, per_pack: int = 16, blob: int = 64 << 10):
    """n_packs device-built packs: (KEY, [IndexPack], {pack id: uint8 device tensor})."""
    from rustic_core_amd.compress import compress_blobs, frame_layout, make_refs
    from rustic_core_amd.device import sha256_device
    from rustic_core_amd.pack import build_packs as build, make_blobs, pack_layout, parse_header
    key = bytes(range(64))
    ctx = _ctx(0)
    rng = np.random.default_rng(7)
    n = n_packs * per_pack
    words = rng.integers(97, 123, (4096, 8), dtype=np.uint8)
    raw = words[rng.integers(0, 4096, n * blob // 8)].reshape(-1)
    d_raw = torch.from_numpy(raw).to(dev)
    offs = np.arange(n, dtype=np.int64) * blob
    refs = torch.from_numpy(np.stack([offs, np.full(n, blob, np.int64)], 1)).to(dev)
    ids = sha256_device(ctx, d_raw, refs).cpu().numpy()
    comp = np.arange(n) % 2 == 1
    c_offs = [int(o) for o in offs[comp]]
    f_offs, ftot = frame_layout([blob] * len(c_offs))
    frames = torch.empty(ftot + 16, dtype=torch.uint8, device=dev)
    flens = compress_blobs(ctx, d_raw.data_ptr(), make_refs(c_offs, [blob] * len(c_offs), f_offs),
                           frames.data_ptr())
    torch.cuda.synchronize()
    # the packer's input: raw blobs where they are, frames behind them
    arena = torch.cat([d_raw, frames])
    in_offs, in_lens = offs.copy(), np.full(n, blob, np.int64)
    in_offs[comp] = len(raw) + np.asarray(f_offs, np.int64)
    in_lens[comp] = np.asarray(flens, np.int64)
    nonces = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    blobs = make_blobs([int(o) for o in in_offs], [int(x) for x in in_lens], list(ids),
                       list(nonces), types=[0] * n,
                       uncompressed=[blob if c else 0 for c in comp])
    groups = [(p * per_pack, per_pack) for p in range(n_packs)]
    packs, total = pack_layout(blobs, groups, list(rng.integers(0, 256, (n_packs, 16), dtype=np.uint8)))
    out = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    build(ctx, key, arena.data_ptr(), blobs, packs, out.data_ptr(), total)
    torch.cuda.synchronize()
    k = Key(key)
    host = out.cpu().numpy()
    index_packs, data = [], {}
    for p in packs:
        o, size = int(p["out_off"]), int(p["size"])
        pack = host[o:o + size].tobytes()
        hlen = int.from_bytes(pack[-4:], "little")
        ip = IndexPack(hashlib.sha256(pack).digest())
        for e in parse_header(k.decrypt_data(pack[-4 - hlen:-4])):
            ip.add(e.id, e.type, e.offset, e.length, e.uncompressed_len or None)
        index_packs.append(ip)
        data[ip.id] = out[o:o + size].clone()
    return k, index_packs, data


def pack_reads():
    from rustic_core_amd.read import check_pack
    k, index_packs, data = build_packs(args.packs)
    size = sum(p.pack_size() for p in index_packs)
    say(f"check_pack for {len(index_packs)} packs, {size / len(index_packs) / 2**20:.2f} MiB each "
        f"({len(index_packs[0].blobs)} blobs, every second one compressed), packs in HBM:")
    found = {}

    def loop():
        found["loop"] = [f for p in index_packs for f in check_pack(k, p, data[p.id])]

    def batch():
        found["batch"] = check.check_pack_batch(k, index_packs, lambda pid: data[pid])
    t = interleaved({"loop over check_pack": loop, "check_pack_batch": batch}, args.reps)
    assert found["loop"] == [] and found["batch"] == []
    for name, s in t.items():
        say(f"  {name:<22} {s * 1e3:9.2f} ms  {size / s / 2**30:7.2f} GiB/s")
    say(f"  the batch takes {'less' if t['check_pack_batch'] < t['loop over check_pack'] else 'NOT less'}"
        f" time than the loop: {t['loop over check_pack'] / t['check_pack_batch']:.2f}x")
    stages = {}
    check.check_pack_batch(k, index_packs, lambda pid: data[pid], stage_times=stages)
    say("  stages of one more batch run (device time by events, ms): " +
        ", ".join(f"{n} {v:.2f}" for n, v in stages.items()))


def main():
    assert torch.cuda.is_available(), "check_prof needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; reps {args.reps} after one warm-up round, "
        "sides interleaved, medians")
    for lg in [int(x) for x in args.log2.split(",")]:
        index_pass(lg, args.pack_blobs, lg <= 20)
    # one workgroup per pack: what small packs cost
    index_pass(20, args.small_pack_blobs, False)
    pack_reads()
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
