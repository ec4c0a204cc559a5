"""Times of prune's plan on the device (rcdc_prune, include/rcdc.h) beside
the same steps in plain Python (rustic_core_amd.prune.HostPrune).

Per size (--log2, default 20,24 entries): a synthetic repository of packs of
--pack blobs with random 32-byte ids generated on the device; --dup-percent
of the entries carry the id of another entry (an id in two packs); the used
ids are half of the distinct ids; a third of the packs are Keep, a third
Repack for ``keep``.

Stages, each the median of --reps after --warmup unmeasured calls, by HIP
events and by the host clock (time.perf_counter around the call and a device
synchronise):
- table:   rcdc_prune_create (the rcdc_dindex over the used ids);
- join:    rcdc_prune_set_entries (pack numbers, the lookup of every entry);
- marking: the counts, the duplicate sort, the rounds and the per-entry
           flags, by the events inside rcdc_prune_mark (its round count and
           the entries that went through the sort are printed);
- sums:    the per-pack sums and their copy to the host, likewise;
- mark:    the whole rcdc_prune_mark call (marking + sums; the host clock
           cannot split them);
- keep:    rcdc_prune_keep.
Baseline in the same run, once per size: HostPrune.set_entries + mark + keep
on the same arrays copied to the host.  Above --host-log2 entries it runs on
the first 2^host-log2 entries (whole packs) against all used ids and is
scaled by the ratio; the line says so.
"""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rustic_core_amd.prune import DevicePrune, HostPrune  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", default="20,24")
ap.add_argument("--host-log2", type=int, default=20)
ap.add_argument("--pack", type=int, default=500)
ap.add_argument("--dup-percent", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
args = ap.parse_args()
assert torch.cuda.is_available(), "prune_prof needs a GPU"
dev = torch.device("cuda:0")


def say(*a):
    print(*a, flush=True)


def timed(fn):
    """(median device ms, median host-clock ms, last result) of fn()."""
    d, h, out = [], [], None
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= args.warmup:
            d.append(e0.elapsed_time(e1))
            h.append((t1 - t0) * 1e3)
    return statistics.median(d), statistics.median(h), out


def line(name, n, d_ms, h_ms, extra=""):
    say(f"{name:<10} device {d_ms:10.3f} ms  host clock {h_ms:10.3f} ms  "
        f"{n / (h_ms * 1e-3) / 1e6:10.2f} M entries/s (host clock){extra}")


say(f"device: {torch.cuda.get_device_name(0)}; packs of {args.pack}, {args.dup_percent}% of the "
    f"entries duplicate another id, half of the ids used; reps {args.reps}, warmup {args.warmup}")
for lg in [int(x) for x in args.log2.split(",")]:
    n = 1 << lg
    g = torch.Generator(device=dev)
    g.manual_seed(lg)
    ids = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=g)
    ndup = int(n * args.dup_percent / 100)
    perm = torch.randperm(n, device=dev, generator=g)
    dst, src = perm[:ndup], perm[ndup:2 * ndup]
    ids[dst] = ids[src]
    original = perm[ndup:]                       # every distinct id once
    used = ids[original[torch.randperm(len(original), device=dev, generator=g)[:len(original) // 2]]]
    used = used.contiguous()
    lens = torch.randint(1, 1 << 20, (n,), dtype=torch.int32, device=dev, generator=g)
    ulens = lens * 2
    ranges = [(f, min(args.pack, n - f)) for f in range(0, n, args.pack)]
    npk = len(ranges)
    kinds = (np.arange(npk) % 3).astype(np.uint8)
    rank = np.arange(npk, dtype=np.uint32)
    say(f"--- 2^{lg}: {n} entries, {npk} packs, {len(used)} used ids")

    made = []

    def create():
        for p in made:
            p.close()
        made[:] = [DevicePrune(used)]
    d_ms, h_ms, _ = timed(create)
    line("table", len(used), d_ms, h_ms, "  (per used id)")
    pr = made[0]
    d_ms, h_ms, _ = timed(lambda: pr.set_entries(ids, lens, ulens, ranges))
    line("join", n, d_ms, h_ms)
    marks, sums = [], []

    def mark():
        out = pr.mark()
        marks.append(out[3].mark_ms)
        sums.append(out[3].sums_ms)
        return out
    d_ms, h_ms, out = timed(mark)
    res = out[3]
    say(f"marking    device {statistics.median(marks[args.warmup:]):10.3f} ms  "
        f"({res.rounds} rounds, {res.dup_entries} entries sorted, {res.missing} ids missing)")
    say(f"sums       device {statistics.median(sums[args.warmup:]):10.3f} ms")
    line("mark", n, d_ms, h_ms)
    d_ms, h_ms, keep = timed(lambda: pr.keep(kinds, rank))
    line("keep", n, d_ms, h_ms)
    say(f"           {int(out[1].sum())} entries used, {int(keep.sum())} kept by the repack")

    nh = min(n, 1 << args.host_log2) // args.pack * args.pack
    part = [r for r in ranges if r[0] + r[1] <= nh]
    h_ids, h_lens, h_ulens = ids[:nh].cpu().numpy(), lens[:nh].cpu().numpy(), ulens[:nh].cpu().numpy()
    h_used = used.cpu().numpy()
    t0 = time.perf_counter()
    hp = HostPrune(h_used)
    hp.set_entries(h_ids, h_lens, h_ulens, part)
    t1 = time.perf_counter()
    hp.mark()
    t2 = time.perf_counter()
    hp.keep(kinds[:len(part)], rank[:len(part)])
    t3 = time.perf_counter()
    scale = n / nh
    note = "" if nh == n else f"  (run on the first {nh} entries, scaled by {scale:.2f})"
    say(f"host: set_entries {1e3 * (t1 - t0) * scale:.0f} ms, mark {1e3 * (t2 - t1) * scale:.0f} ms, "
        f"keep {1e3 * (t3 - t2) * scale:.0f} ms; {nh / (t3 - t0) / 1e6:.3f} M entries/s{note}")
    pr.close()
    del ids, used, lens, ulens
