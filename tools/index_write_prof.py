"""Writing index files from the device: index_write.write_json
(rcdc_index_write) and save_index_files beside today's host path,
IndexFile.to_json + save_index_file per file, on the same entries.

Per size (--log2, default 20,24 entries): the synthetic index of
tools/index_load_prof.py -- files of 50 000 blobs (index.MAX_COUNT) in packs
of --pack-blobs blobs, random ids, an 8-digit offset, a 6-digit length and a
7-digit uncompressed length per blob, a time per pack -- as entry arrays in
HBM and one record per pack.
- write_json: the text of all files into one arena;
- write_json + save_index_files: the text, then per file 2 || zstd frame,
  sealed, and the SHA-256 of the sealed bytes (version 2);
- host: save_index_file(key, IndexFile) for every file, the IndexFile objects
  built beforehand and not timed; run once, on the first --host-files files
  (a stated fraction at 2^24, scaled to all files in the "scaled" figure);
- copy: a device-to-device copy of as many bytes as write_json wrote, the
  emit pass's ceiling.
Wall times are time.perf_counter around the call and a device synchronise,
the median of --reps after --warmup unmeasured calls.  The stage lines are
HIP events around the stage's device calls, from one more run.
"""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rustic_core_amd.crypto import Key  # noqa: E402
from rustic_core_amd.index import (MAX_COUNT, IndexBlob, IndexFile, IndexPack,  # noqa: E402
                                   save_index_file)
from rustic_core_amd.index_write import (FileRecord, PackRecord, file_records,  # noqa: E402
                                         pack_records, save_index_files, write_json)

ap = argparse.ArgumentParser()
ap.add_argument("--log2", default="20,24")
ap.add_argument("--pack-blobs", type=int, default=500)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--host-files", type=int, default=21, help="files the host path runs on")
ap.add_argument("--only-write", action="store_true",
                help="write_json alone, for a kernel trace of its launches")
args = ap.parse_args()
dev = torch.device("cuda:0")
TIME = "2024-05-06T07:08:09.123456789+02:00"


def say(*a):
    print(*a, flush=True)


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


def evented(fn, reps, warmup):
    """Device time of fn by HIP events, milliseconds."""
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t), min(t), max(t)


def host_files(ids, offs, lens, ulens, n_files, per_pack):
    out = []
    for f in range(n_files):
        packs = []
        for k in range(MAX_COUNT // per_pack):
            e0 = f * MAX_COUNT + k * per_pack
            pid = ids[e0].tobytes()[::-1]
            packs.append(IndexPack(pid, [IndexBlob(ids[e].tobytes(), (f % 4 == 3) * 1, int(offs[e]),
                                                   int(lens[e]), int(ulens[e]))
                                         for e in range(e0, e0 + per_pack)], TIME))
        out.append(IndexFile(packs=packs))
    return out


def main():
    assert torch.cuda.is_available(), "index_write_prof needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; files of {MAX_COUNT} blobs, packs of "
        f"{args.pack_blobs}; reps {args.reps}, warmup {args.warmup}")
    key = Key(bytes(range(64)))
    for lg in [int(x) for x in args.log2.split(",")]:
        rng = np.random.default_rng(lg)
        n_files = -(-(1 << lg) // MAX_COUNT)
        n = n_files * MAX_COUNT
        ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        offs = rng.integers(10_000_000, 99_999_999, n).astype(np.uint32)
        lens = rng.integers(100_000, 999_999, n).astype(np.uint32)
        ulens = rng.integers(1_000_000, 9_999_999, n).astype(np.uint32)
        per_file = MAX_COUNT // args.pack_blobs
        packs = [PackRecord(ids[e0].tobytes()[::-1], ((e0 // MAX_COUNT) % 4 == 3) * 1, e0,
                            args.pack_blobs, TIME) for e0 in range(0, n, args.pack_blobs)]
        files = [FileRecord(f * per_file, per_file) for f in range(n_files)]
        p_recs, f_recs = pack_records(packs), file_records(files)
        d = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)
             for a in (ids, offs, lens, ulens)]
        w = write_json(*d, p_recs, f_recs)
        total = int(sum(w.lens))
        say(f"--- 2^{lg}: {n_files} files, {n} entries, {total / 1e6:.1f} MB of JSON "
            f"({total / n:.1f} B per blob)")
        if args.only_write:
            for _ in range(args.reps):
                write_json(*d, p_recs, f_recs)
            continue
        # the host path on the same entries, and the bytes agree
        hf = min(args.host_files, n_files)
        objs = host_files(ids, offs, lens, ulens, hf, args.pack_blobs)
        t0 = time.perf_counter()
        saved = [save_index_file(key, f) for f in objs]
        host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        texts = [f.to_json() for f in objs]
        json_s = time.perf_counter() - t0
        got = w.data.cpu().numpy()
        for i, t in enumerate(texts):
            o = int(w.offs[i])
            assert got[o:o + int(w.lens[i])].tobytes() == t, i
        del got, objs, texts
        host_all = host_s * n_files / hf
        say(f"host: save_index_file x {hf} of {n_files} files   {host_s * 1e3:10.1f} ms "
            f"(to_json alone {json_s * 1e3:.1f} ms; sealed {sum(len(s) for _, s in saved) / 1e6:.1f} MB)"
            f"  scaled to all files {host_all * 1e3:10.1f} ms  {n / host_all / 1e6:8.3f} M entries/s")
        del w
        rows = [("write_json", clocked(lambda: write_json(*d, p_recs, f_recs), args.reps, args.warmup))]

        def both():
            ww = write_json(*d, p_recs, f_recs)
            return save_index_files(key, ww)
        rows.append(("write_json + save_index_files", clocked(both, args.reps, args.warmup)))
        for name, (med, lo, hi) in rows:
            say(f"{name:30s} median {med * 1e3:9.1f} ms  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  "
                f"{n / med / 1e6:8.2f} M entries/s  {total / med / 1e9:7.3f} GB/s of JSON  "
                f"{host_all / med:8.1f} x host")
        stages = {}
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ww = write_json(*d, p_recs, f_recs)
        b.record()
        b.synchronize()
        stages["write"] = a.elapsed_time(b)
        ids_, sealed, s_offs, s_lens = save_index_files(key, ww, stage_times=stages)
        say("device time by stage (ms): " +
            ", ".join(f"{k} {stages.get(k, 0.0):.2f}" for k in ("write", "compress", "seal", "sha256")) +
            f"; {int(sum(s_lens)) / 1e6:.1f} MB sealed")
        src = ww.raw[:total]
        dst = torch.empty_like(src)
        med, lo, hi = evented(lambda: dst.copy_(src), args.reps, args.warmup)
        wm = evented(lambda: write_json(*d, p_recs, f_recs), args.reps, args.warmup)[0]
        say(f"copy of {total / 1e6:.1f} MB, device to device: median {med:.3f} ms "
            f"({total / med / 1e6:.1f} GB/s written); write_json by events {wm:.3f} ms "
            f"({total / wm / 1e6:.1f} GB/s): {med / wm:.2f} of the copy's rate")
        del ww, src, dst, sealed, d


if __name__ == "__main__":
    main()
