"""Rates of the blob index in device memory (rcdc_dindex, include/rcdc.h)
beside the host paths it stands in for.

Per index size (--log2, default 20,24,26 entries of random 32-byte ids with
locations, generated on the device):
- build: entries/s of one rcdc_dindex_add of all entries into an index
  created with reserve_entries = size, and of adds of 2^20 entries into an
  index created empty (it grows and rebuilds its table on the way);
- lookup: ids/s of rcdc_dindex_lookup over --queries ids and over a 2^16
  batch, half of them in the index, half not, shuffled;
- first_new: ids/s of rcdc_dindex_first_new over the same batches, and the
  whole dedup step as ingest runs it (DeviceIndex.first_new + the flags'
  copy to the host).
Device times are HIP events around the call, the median of --reps after
--warmup unmeasured calls; "host clock" is time.perf_counter around the
call and a device synchronise.

Host paths, at sizes up to --host-log2 (the Python set of 2^26 ids takes
about 8 GB of host memory and 17 s to build):
- ingest.first_occurrences over the same 2^16 batch against a Python set of
  the index's ids, including the copy of the ids to the host, as
  DeviceIngest.end does with indexed=set;
- the reference's method on one thread: the ids sorted (np.sort of the
  32-byte strings: IndexCollector::into_index) and np.searchsorted plus an
  equality test per query (binary_search_by_key).
"""
import argparse
import ctypes
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rustic_core_amd import _lib  # noqa: E402
from rustic_core_amd.crypto import _ctx  # noqa: E402
from rustic_core_amd.dindex import DATA, DEVICE_PTRS, DeviceIndex  # noqa: E402
from rustic_core_amd.ingest import first_occurrences  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", default="20,24,26")
ap.add_argument("--host-log2", type=int, default=26, help="largest size the host paths run at")
ap.add_argument("--queries", type=int, default=1 << 22)
ap.add_argument("--batch", type=int, default=1 << 16)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
assert torch.cuda.is_available(), "index_prof needs a GPU"
dev = torch.device("cuda:0")
L = _lib.lib()
ctx = _ctx(0)


def say(*a):
    print(*a, flush=True)


def ck(st):
    assert st == 0, _lib.last_error()


def timed(fn, reps=None, warmup=None):
    """(median device seconds, median host-clock seconds) of fn()."""
    reps = args.reps if reps is None else reps
    for _ in range(args.warmup if warmup is None else warmup):
        fn()
    torch.cuda.synchronize()
    d, h = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        h.append(time.perf_counter() - t0)
        d.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(d), statistics.median(h)


def rate(n, s):
    return f"{n / s / 1e6:9.1f} M/s ({s * 1e3:9.3f} ms)"


def raw_index(reserve):
    h = ctypes.c_void_p()
    ck(L.rcdc_dindex_create(ctx.handle, reserve, ctypes.byref(h)))
    return h


def mixed(ids, n, gen):
    """n queries: half rows of ids, half fresh random ids, shuffled."""
    hit = ids[torch.randint(0, ids.shape[0], (n // 2,), device=dev, generator=gen)]
    miss = torch.randint(0, 256, (n - n // 2, 32), dtype=torch.uint8, device=dev, generator=gen)
    q = torch.cat([hit, miss])
    return q[torch.randperm(n, device=dev, generator=gen)].contiguous()


say(f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}; reps {args.reps}, warm-up "
    f"{args.warmup}; queries {args.queries}, batch {args.batch}")
for lg in [int(x) for x in args.log2.split(",")]:
    N = 1 << lg
    gen = torch.Generator(device=dev)
    gen.manual_seed(lg)
    ids = torch.empty((N, 32), dtype=torch.uint8, device=dev)
    for a in range(0, N, 1 << 22):  # random ids: what SHA-256 output looks like to the table
        ids[a:a + (1 << 22)].random_(0, 256, generator=gen)
    locs = torch.randint(0, 1 << 30, (N, 4), dtype=torch.int32, device=dev, generator=gen)
    say(f"\n== 2^{lg} = {N} entries ==")

    # ---- build ----------------------------------------------------------------
    def build_reserved():
        h = raw_index(N)
        ck(L.rcdc_dindex_add(h, ids.data_ptr(), locs.data_ptr(), N, DEVICE_PTRS, None))
        L.rcdc_dindex_destroy(h)

    def build_grown():
        h = raw_index(0)
        step = 1 << 20
        for a in range(0, N, step):
            m = min(step, N - a)
            ck(L.rcdc_dindex_add(h, ids[a:a + m].data_ptr(), locs[a:a + m].data_ptr(), m,
                                 DEVICE_PTRS, None))
        L.rcdc_dindex_destroy(h)

    reps_b = 3 if lg >= 24 else args.reps
    _, hb = timed(build_reserved, reps_b, 1)
    say(f"build, one add, reserved      : {rate(N, hb)}  host clock, create + add + destroy")
    _, hg = timed(build_grown, reps_b, 1)
    say(f"build, adds of 2^20, from empty: {rate(N, hg)}  host clock, with the table's rebuilds")

    # the index the lookups run against: through DeviceIndex, id-only entries
    dx = DeviceIndex(0)
    t0 = time.perf_counter()
    dx.add_ids(ids)
    torch.cuda.synchronize()
    say(f"DeviceIndex.add_ids (id-only)  : {rate(N, time.perf_counter() - t0)}  host clock, first call")
    assert dx.size(DATA) == N
    h = dx._t[DATA].handle

    # ---- lookup and first_new -----------------------------------------------------
    for nq in (args.queries, args.batch):
        q = mixed(ids, nq, gen)
        hits = torch.empty((nq, 6), dtype=torch.int32, device=dev)
        new = torch.empty(nq, dtype=torch.uint8, device=dev)
        d, hh = timed(lambda: ck(L.rcdc_dindex_lookup(h, q.data_ptr(), nq, hits.data_ptr(), None)))
        found = int((hits[:, 1] != 0).sum())
        say(f"lookup    of {nq:8d} ids      : {rate(nq, d)}  device; {rate(nq, hh)} host clock; "
            f"{found} found")
        d, hh = timed(lambda: ck(L.rcdc_dindex_first_new(h, q.data_ptr(), nq, None, new.data_ptr(),
                                                          None)))
        say(f"first_new of {nq:8d} ids      : {rate(nq, d)}  device; {rate(nq, hh)} host clock; "
            f"{int(new.sum())} new")
    # the dedup step as DeviceIngest.end runs it: flags back on the host
    qb = mixed(ids, args.batch, gen)
    _, hd = timed(lambda: dx.first_new(qb).cpu().numpy())
    say(f"dedup step, device index, batch {args.batch}: {rate(args.batch, hd)}  host clock, "
        f"DeviceIndex.first_new + flags to the host")
    dev_new = dx.first_new(qb).cpu().numpy()

    # ---- the host paths ----------------------------------------------------------------
    if lg > args.host_log2:
        say(f"host paths: not measured at 2^{lg} (--host-log2 {args.host_log2})")
        dx.close()
        del ids, locs
        torch.cuda.empty_cache()
        continue
    t0 = time.perf_counter()
    host_ids = ids.cpu().numpy()
    buf = host_ids.tobytes()
    known = {buf[i:i + 32] for i in range(0, len(buf), 32)}
    del buf
    say(f"host: Python set of the ids built in {time.perf_counter() - t0:.1f} s "
        f"({rate(N, time.perf_counter() - t0)})")

    def set_path():
        a = qb.cpu().numpy()  # the ids' copy to the host is part of the path
        return first_occurrences(a, np.arange(len(a)), known)

    _, hs = timed(set_path, 5, 1)
    say(f"dedup step, Python set,   batch {args.batch}: {rate(args.batch, hs)}  host clock, "
        f"ids to the host + first_occurrences")
    assert (set_path() == dev_new).all(), "device and host dedup differ"
    say(f"  device dedup step / set path: {hs / hd:.1f}x faster" if hd < hs else
        f"  device dedup step / set path: {hd / hs:.1f}x SLOWER")
    del known
    t0 = time.perf_counter()
    s = np.sort(host_ids.view("S32").ravel())
    ts = time.perf_counter() - t0
    say(f"host: np.sort of the 32-byte ids  : {rate(N, ts)}  one thread (the reference's build)")
    for nq in (args.queries, args.batch):
        qh = mixed(ids, nq, gen).cpu().numpy().view("S32").ravel()

        def search():
            p = np.searchsorted(s, qh)
            return s[np.minimum(p, N - 1)] == qh

        t0 = time.perf_counter()
        f = search()
        th = time.perf_counter() - t0
        say(f"host: searchsorted of {nq:8d} ids: {rate(nq, th)}  one thread; {int(f.sum())} found")
    dx.close()
    del ids, locs, s, host_ids
    torch.cuda.empty_cache()
