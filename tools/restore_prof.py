#!/usr/bin/env python3
"""Rates of the restore path on the device.

Place alone: rcdc_place_blobs over --gib GiB of blobs with one destination
each, at random alignments on both sides -- with flags 0 and zero NULL, with
the zero flags, and with RCDC_PLACE_SKIP_ZERO on data whose blobs are 25 %
all-zero -- against rcdc_copy_ranges over the identical ranges (the range
copy the library had before) and a torch copy_ of one contiguous buffer of
the same size (the ceiling).  One row for blobs of 0.5-8 MiB, one for 16 KiB
blobs.  Then restore_contents end to end over what the native ingest engine
backed up (packs in HBM).

Every figure is the median of --reps timed calls after a warm-up, with min
and max; the variants alternate inside each repetition.  The calls return
once their work has run, so the host clock around a call (after a device
synchronise) is the call's time: tile list, uploads and launches included.
Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GIB = 1 << 30


def _layout(rng, total, lo, hi):
    """Blobs of lo..hi bytes up to `total`: (in_off, len, out_off), sources
    in order, destinations in a shuffled order, every offset at a random
    alignment."""
    lens = []
    left = total
    while left > 0:
        n = int(rng.integers(lo, hi + 1)) if hi > lo else lo
        n = min(n, left)
        lens.append(n)
        left -= n
    lens = np.array(lens, np.int64)
    n = len(lens)
    in_off = np.cumsum(np.concatenate([[0], lens[:-1] + 16])) + rng.integers(0, 16, n)
    order = rng.permutation(n)
    out_off = np.zeros(n, np.int64)
    out_off[order] = np.cumsum(np.concatenate([[0], lens[order][:-1] + 16])) + rng.integers(0, 16, n)
    return in_off, lens, out_off, int(lens.sum() + 16 * n + 64)


def _time(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


def _fmt(nbytes, ts):
    r = sorted(nbytes / t / GIB for t in ts)
    return f"{statistics.median(r):8.1f} GiB/s  (min {r[0]:.1f}, max {r[-1]:.1f})"


def place_rows(ctx, total, lo, hi, reps, label, out):
    import torch
    from rustic_core_amd import _lib
    from rustic_core_amd.pack import PLACE_BLOB, PLACE_DEST, copy_ranges
    rng = np.random.default_rng(5)
    in_off, lens, out_off, span = _layout(rng, total, lo, hi)
    n = len(lens)
    dev = torch.device("cuda", 0)
    src = torch.randint(0, 256, (min(span, 256 << 20),), dtype=torch.uint8, device=dev)
    src = src.repeat((span + src.numel() - 1) // src.numel())[:span].contiguous()
    src_z = src.clone()   # every fourth blob all zero
    for k in range(0, n, 4):
        src_z[int(in_off[k]):int(in_off[k] + lens[k])] = 0
    dst = torch.zeros(span, dtype=torch.uint8, device=dev)
    dst2 = torch.zeros(span, dtype=torch.uint8, device=dev)
    blobs = np.zeros(n, PLACE_BLOB)
    blobs["in_off"], blobs["len"], blobs["dest0"], blobs["ndests"] = in_off, lens, np.arange(n), 1
    dests = np.zeros(n, PLACE_DEST)
    dests["out_off"] = out_off
    L = _lib.lib()
    il = np.array([span], np.uint64)
    zero = np.zeros(n, np.uint8)

    def place(s, d, flags, z):
        ins = (ctypes.c_void_p * 1)(s.data_ptr())
        outs = (ctypes.c_void_p * 1)(d.data_ptr())
        st = L.rcdc_place_blobs(ctx.handle, ctypes.cast(ins, ctypes.c_void_p), il.ctypes.data, 1,
                                blobs.ctypes.data, n, dests.ctypes.data, n,
                                ctypes.cast(outs, ctypes.c_void_p), il.ctypes.data, 1, flags,
                                z.ctypes.data if z is not None else None, None)
        if st:
            raise RuntimeError(_lib.last_error())

    variants = [
        ("place_blobs, flags 0, zero NULL", lambda: place(src, dst, 0, None)),
        ("place_blobs, zero flags", lambda: place(src, dst, 0, zero)),
        ("place_blobs, SKIP_ZERO, 25 % zero blobs", lambda: place(src_z, dst, 1, zero)),
        ("copy_ranges, the same ranges", lambda: copy_ranges(ctx, [src.data_ptr()], 0, in_off, lens,
                                                             out_off, dst2.data_ptr())),
        ("torch copy_, one contiguous buffer", lambda: dst2.copy_(src)),
    ]
    sync = torch.cuda.synchronize
    # the two range copies agree before anything is timed
    place(src, dst, 0, None)
    variants[3][1]()
    sync()
    if not torch.equal(dst, dst2):
        raise RuntimeError("place_blobs and copy_ranges disagree")
    place(src_z, dst, 0, zero)
    want = np.zeros(n, np.uint8)
    want[::4] = 1
    if not np.array_equal(zero, want):
        raise RuntimeError("zero flags are wrong")
    times = {name: [] for name, _ in variants}
    for name, fn in variants:   # warm-up
        _time(fn, sync)
    for _ in range(reps):
        for name, fn in variants:
            times[name].append(_time(fn, sync))
    nbytes = int(lens.sum())
    out.append(f"{label}: {n} blobs, {nbytes / GIB:.2f} GiB, {reps} repetitions")
    for name, _ in variants:
        out.append(f"  {name:42s} {_fmt(nbytes, times[name])}")


def restore_row(ctx, total, reps, out):
    """restore_contents over a backup of the native ingest engine: random
    files with zero runs, level 0, packs as device tensors."""
    import torch
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.index import IndexFile, IndexPack
    from rustic_core_amd.native_ingest import NativeIngest
    from rustic_core_amd.restore import RestorePlan, from_packs, index_lookup, restore_contents
    key = bytes(range(7, 71))
    rng = np.random.default_rng(6)
    nfiles = 4
    files = []
    for _ in range(nfiles):
        f = rng.integers(0, 256, total // nfiles, dtype=np.uint8)
        for _ in range(4):   # a few zero runs of 4 MiB
            p = int(rng.integers(0, max(f.size - (4 << 20), 1)))
            f[p:p + (4 << 20)] = 0
        files.append(f)
    ing = NativeIngest(ctx, key, level=0, batch_bytes=256 << 20)
    try:
        for i, f in enumerate(files):
            ing.add(i, f)
        ing.finish()
        dev = torch.device("cuda", 0)
        packs = {p["id"]: torch.frombuffer(bytearray(p["data"]), dtype=torch.uint8).to(dev)
                 for p in ing.packs}
        index_files = []
        for p in ing.packs:
            ip = IndexPack(p["id"])
            for bid, off, ln, ulen, tpe in p["blobs"]:
                ip.add(bid, tpe, off, ln, ulen or None)
            index_files.append(IndexFile([ip]))
        ids = [[bytes(x) for x in ing.files[i][1]] for i in range(nfiles)]
    finally:
        ing.close()
    index = index_lookup(index_files)
    plan = RestorePlan()
    t0 = time.perf_counter()
    for i, f in enumerate(files):
        plan.add_file(f"f{i}", f.size, ids[i], index)
    t_plan = time.perf_counter() - t0
    k = Key(key)
    sync = torch.cuda.synchronize
    res = restore_contents(k, plan, from_packs(packs))   # warm-up, and the check
    sync()
    for t, f in zip(res.files, files):
        if not np.array_equal(t.cpu().numpy(), f):
            raise RuntimeError("restore_contents returned other bytes")
    del res
    rows = {"restore_contents": [], "restore_contents, sparse": []}
    for _ in range(reps):
        rows["restore_contents"].append(
            _time(lambda: restore_contents(k, plan, from_packs(packs)), sync))
        rows["restore_contents, sparse"].append(
            _time(lambda: restore_contents(k, plan, from_packs(packs), sparse=True), sync))
    nbytes = plan.restore_size
    out.append(f"end to end: {nfiles} files, {nbytes / GIB:.2f} GiB, {len(plan.r)} blobs in "
               f"{len(packs)} packs (level 0, packs in HBM), {len(plan.pack_reads())} reads; "
               f"plan {t_plan * 1e3:.0f} ms")
    for name, ts in rows.items():
        out.append(f"  {name:42s} {_fmt(nbytes, ts)}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gib", type=float, default=4.0, help="bytes placed per call, in GiB")
    ap.add_argument("--e2e-gib", type=float, default=1.0, help="bytes backed up and restored")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "restore.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("restore_prof.py needs a GPU")
    if a.reps < 3:
        sys.exit("--reps must be at least 3")
    from rustic_core_amd.crypto import _ctx
    ctx = _ctx(0)
    out = [f"restore_prof.py on {torch.cuda.get_device_name(0)}"]
    total = int(a.gib * GIB)
    place_rows(ctx, total, 512 << 10, 8 << 20, a.reps, "blobs of 0.5-8 MiB", out)
    torch.cuda.empty_cache()
    place_rows(ctx, total, 16 << 10, 16 << 10, a.reps, "blobs of 16 KiB", out)
    torch.cuda.empty_cache()
    if a.e2e_gib > 0:
        restore_row(ctx, int(a.e2e_gib * GIB), a.reps, out)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
