"""Pack headers on the device, stage by stage: open (Key.open_blobs), parse
(headers.parse_headers, rcdc_pack_header_parse), add (rcdc_dindex_add on the
parser's device arrays) and index write (index_write.write_json over the same
arrays, then save_index_files: compress, seal, hash) -- what repair index
--read-all and index_checked do behind their reads -- beside the host loop on
the same bytes: per header Key.decrypt_data, pack.parse_header and
index.Indexer with IndexFile.to_json.

Three synthetic shapes:
- data: 2^--log2-data headers (default 15) of about 32 entries, as data packs
  have them; half of the entries compressed;
- tree: --tree-headers headers (default 256) of about 4 000 entries;
- one: one header of 65 535 entries.

Stage times are HIP events around each stage on the current stream, the
median, min and max of --reps after --warmup unmeasured rounds; a round runs
all stages once.  A stage's time holds the host work of its call too (the
stream waits for it); "records (host)" is the one piece of host work between
the stages, the numpy records of the packs and files for write_json, by
time.perf_counter.  The kernel lines are device times of one more parse under
torch.profiler (kernels named rcdc_ph_*).  The host loop runs over --host-headers headers of each shape
(it is the same work per header) and is clocked with time.perf_counter; its
decrypt_data goes through the device one header at a time, which is what the
per-pack read path of this project costs.
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
from rustic_core_amd.headers import OK, parse_headers  # noqa: E402
from rustic_core_amd.index import Indexer, IndexPack  # noqa: E402
from rustic_core_amd.index_write import (FileRecord, PackRecord, file_records,  # noqa: E402
                                         pack_records, save_index_files, write_json)
from rustic_core_amd.pack import parse_header  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-data", type=int, default=15)
ap.add_argument("--tree-headers", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-headers", type=int, default=64)
args = ap.parse_args()
dev = torch.device("cuda:0")
STAGES = ("open", "parse", "add", "records (host)", "write", "save")


def say(*a):
    print(*a, flush=True)


def make_headers(rng, counts, tree: bool):
    """Plain headers with ``counts[i]`` entries each, about half of them
    compressed, lengths that never overflow: (list of byte arrays, entries)."""
    n = int(sum(counts))
    rows = np.zeros((n, 41), np.uint8)
    comp = rng.integers(0, 2, n).astype(np.uint8)
    rows[:, 0] = 2 * comp + (1 if tree else 0)
    rows[:, 1:5] = rng.integers(1, 60000, n).astype("<u4").view(np.uint8).reshape(n, 4)
    rows[:, 5:9] = rng.integers(1, 1 << 20, n).astype("<u4").view(np.uint8).reshape(n, 4)
    rows[:, 9:] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    keep = np.ones((n, 41), bool)
    keep[comp == 0, 5:9] = False
    flat = rows[keep]
    sizes = np.where(comp == 1, 41, 37)
    ends = np.cumsum(sizes)[np.cumsum(counts) - 1]
    starts = np.concatenate([[0], ends[:-1]])
    return [flat[a:b] for a, b in zip(starts, ends)], n


def seal_all(key, plains):
    lens = np.array([len(p) for p in plains], np.int64)
    in_offs = np.concatenate([[0], np.cumsum((lens + 15) // 16 * 16)[:-1]]).astype(np.uint64)
    host = np.zeros(int(in_offs[-1]) + int(lens[-1]) + 64, np.uint8)
    for o, p in zip(in_offs, plains):
        host[int(o):int(o) + len(p)] = p
    out_offs, total = sealed_layout(lens)
    d_in = torch.from_numpy(host).to(dev)
    d_out = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    nonces = np.random.default_rng(1).integers(0, 256, (len(plains), 16), dtype=np.uint8)
    key.seal_blobs(d_in.data_ptr(), make_refs(in_offs, lens, out_offs, nonces), d_out.data_ptr(),
                   torch.cuda.current_stream(dev).cuda_stream, _ctx(0))
    torch.cuda.synchronize()
    return d_out, np.asarray(out_offs, np.int64), lens + 32


class Clock:
    def __init__(self):
        self.ms = {s: [] for s in STAGES}

    def stage(self, name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream(dev))
        out = fn()
        b.record(torch.cuda.current_stream(dev))
        b.synchronize()
        self.ms[name].append(a.elapsed_time(b))
        return out


def device_round(key, clock, sealed, s_offs, s_lens, pack_ids):
    stream = torch.cuda.current_stream(dev).cuda_stream
    p_lens = s_lens - 32
    p_offs = np.concatenate([[0], np.cumsum((p_lens + 15) // 16 * 16)[:-1]]).astype(np.int64)
    plain = torch.empty(int(p_offs[-1]) + int(p_lens[-1]) + 64, dtype=torch.uint8, device=dev)
    st = clock.stage("open", lambda: key.open_blobs(sealed.data_ptr(),
                                                    make_refs(s_offs, s_lens, p_offs),
                                                    plain.data_ptr(), stream, _ctx(0)))
    assert not st.any()
    res = clock.stage("parse", lambda: parse_headers(plain, p_offs, p_lens))
    assert (res.headers["status"] == OK).all()
    dx = DeviceIndex(0)

    def add():
        for t in (0, 1):
            n = res.entries[t]
            if n:
                dx._add(dx._t[t], res.ids[t][:n], res.locs[t][:n], 1)
    clock.stage("add", add)
    assert len(dx) == sum(res.entries)
    dx.close()
    t = int(res.headers["type"][0])
    packs = [PackRecord(i, t, int(h["first"]), int(h["count"]))
             for i, h in zip(pack_ids, res.headers)]
    # files of 50 000 entries or more, as Indexer closes them
    files, first, count = [], 0, 0
    for k, p in enumerate(packs):
        count += p.count
        if count >= 50000 or k == len(packs) - 1:
            files.append(FileRecord(first, k + 1 - first))
            first, count = k + 1, 0
    ids, offs, lens, ulens = res.columns(t)
    t0 = time.perf_counter()
    recs = (pack_records(packs), file_records(files))  # host: one numpy record per pack
    clock.ms["records (host)"].append((time.perf_counter() - t0) * 1e3)
    written = clock.stage("write", lambda: write_json(ids, offs, lens, ulens, *recs))
    clock.stage("save", lambda: save_index_files(key, written))
    return sum(res.entries), int(written.total), len(files)


def kernels(fn):
    """Device time per rcdc_ph_* kernel of one call of fn."""
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total)
                for e in prof.key_averages() if "rcdc_ph_" in e.key]
    except Exception as e:  # the profiler is a convenience, the clocks above are the result
        say(f"  (no kernel times: {e})")
        return
    if not rows:
        say("  (the profiler saw no rcdc_ph_* kernel)")
        return
    total = sum(t for _, t in rows)
    for k, t in sorted(rows, key=lambda r: -r[1]):
        say(f"    {k.split('(')[0]:32s} {t / 1e3:9.3f} ms  {100 * t / total:5.1f} %")
    say(f"    {'all rcdc_ph_* kernels of a parse':32s} {total / 1e3:9.3f} ms")


def host_loop(key, sealed_host, pack_ids):
    saved, entries = [], 0
    ix = Indexer(lambda f: saved.append(len(f.to_json())) or b"")
    t0 = time.perf_counter()
    for pid, s in zip(pack_ids, sealed_host):
        p = IndexPack(pid)
        for b in parse_header(key.decrypt_data(s)):
            p.add(b.id, b.type, b.offset, b.length, b.uncompressed_len or None)
        entries += len(p.blobs)
        ix.add(p)
    ix.finalize()
    return time.perf_counter() - t0, entries


def shape(key, name, plains, entries):
    n = len(plains)
    nbytes = sum(len(p) for p in plains)
    pack_ids = [hashlib.sha256(b"pack %d" % k).digest() for k in range(n)]
    sealed, s_offs, s_lens = seal_all(key, plains)
    say(f"--- {name}: {n} headers, {entries} entries, {nbytes / 1e6:.2f} MB of plain header")
    clock = Clock()
    for _ in range(args.warmup):
        device_round(key, Clock(), sealed, s_offs, s_lens, pack_ids)
    for _ in range(args.reps):
        got, text, nfiles = device_round(key, clock, sealed, s_offs, s_lens, pack_ids)
    assert got == entries
    total = 0.0
    for s in STAGES:
        v = clock.ms[s]
        med = statistics.median(v)
        total += med
        say(f"  {s:14s} median {med:9.3f} ms  (min {min(v):.3f}, max {max(v):.3f})  "
            f"{entries / med / 1e3:9.2f} M entries/s")
    say(f"  {'all':14s} sum of medians {total:9.3f} ms  {entries / total / 1e3:9.2f} M entries/s; "
        f"{nfiles} index files, {text / 1e6:.2f} MB of JSON")
    p_lens = s_lens - 32
    p_offs = np.concatenate([[0], np.cumsum((p_lens + 15) // 16 * 16)[:-1]]).astype(np.int64)
    plain = torch.empty(int(p_offs[-1]) + int(p_lens[-1]) + 64, dtype=torch.uint8, device=dev)
    key.open_blobs(sealed.data_ptr(), make_refs(s_offs, s_lens, p_offs), plain.data_ptr(),
                   torch.cuda.current_stream(dev).cuda_stream, _ctx(0))
    kernels(lambda: parse_headers(plain, p_offs, p_lens))
    del plain
    k = min(n, args.host_headers)
    host = sealed.cpu().numpy()
    sealed_host = [host[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(s_offs[:k], s_lens[:k])]
    host_loop(key, sealed_host[:2], pack_ids[:2])  # warm-up
    t, e = host_loop(key, sealed_host, pack_ids[:k])
    say(f"  host loop over {k} headers: {t * 1e3:9.3f} ms, {t / k * 1e3:.3f} ms per header, "
        f"{e / t / 1e6:.3f} M entries/s; for all {n} headers at that rate: {t / k * n * 1e3:.1f} ms")


def main():
    assert torch.cuda.is_available(), "pack_header_prof needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; reps {args.reps}, warmup {args.warmup}; stage "
        "times by HIP events; the host loop is decrypt_data + parse_header + Indexer per header "
        "on one thread")
    key = Key(bytes(range(64)))
    rng = np.random.default_rng(23)
    n = 1 << args.log2_data
    plains, e = make_headers(rng, rng.integers(24, 41, n), tree=False)
    shape(key, f"data (2^{args.log2_data} headers x ~32 entries)", plains, e)
    plains, e = make_headers(rng, rng.integers(3500, 4501, args.tree_headers), tree=True)
    shape(key, f"tree ({args.tree_headers} headers x ~4000 entries)", plains, e)
    plains, e = make_headers(rng, np.array([65535]), tree=True)
    shape(key, "one (1 header x 65535 entries)", plains, e)


if __name__ == "__main__":
    main()
