"""Loading index files into the device index: DeviceIndex.load and
DeviceIndex.extend_json (rcdc_index_parse) beside today's host path,
IndexFile.from_json + DeviceIndex.from_index_files, on the same bytes.

Per size (--log2, default 20,24 entries): synthetic index files of 50 000
blobs each (index.MAX_COUNT) in packs of --pack-blobs blobs, random ids, the
compact form serde_json writes, sealed as a version-2 repository saves them
(2 || zstd frame).
- host: from_json of every file's text, then from_index_files (the text is
  already decrypted and decoded: the host path's best case);
- extend_json: the text uploaded once, then parse + add;
- load: the sealed files uploaded, opened, decoded, parsed, added.
Times are time.perf_counter around the call and a device synchronise, the
median of --reps after --warmup unmeasured calls (the host path, minutes at
2^24, runs --host-reps times and is not warmed up).  The stage lines are HIP
events around the stage's device calls (DeviceIndex.stage_times), from one
more run of load: open, decode, parse, add.
"""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rustic_core_amd.crypto import Key  # noqa: E402
from rustic_core_amd.dindex import DATA, TREE, DeviceIndex  # noqa: E402
from rustic_core_amd.index import MAX_COUNT, IndexFile, encrypt_file  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2", default="20,24")
ap.add_argument("--pack-blobs", type=int, default=500)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--host-reps", type=int, default=1)
ap.add_argument("--host-log2", type=int, default=24, help="largest size the host path runs at")
args = ap.parse_args()
dev = torch.device("cuda:0")
HEXD = np.frombuffer(b"0123456789abcdef", np.uint8)


def say(*a):
    print(*a, flush=True)


def hexed(ids: np.ndarray) -> np.ndarray:
    out = np.empty(ids.shape[:-1] + (ids.shape[-1] * 2,), np.uint8)
    out[..., 0::2] = HEXD[ids >> 4]
    out[..., 1::2] = HEXD[ids & 15]
    return out


def digits(v: np.ndarray, width: int) -> np.ndarray:
    """v (each with exactly ``width`` decimal digits) as ASCII."""
    out = np.empty(v.shape + (width,), np.uint8)
    for k in range(width):
        out[..., width - 1 - k] = 0x30 + (v // 10 ** k) % 10
    return out


def make_file(rng, n_blobs: int, per_pack: int, tree: bool) -> bytes:
    """One index file as serde_json writes it; every number has a fixed
    number of digits, so the rows are columns of one byte matrix."""
    assert n_blobs % per_pack == 0
    tpe = b"tree" if tree else b"data"
    parts = [b'{"id":"', None, b'","type":"' + tpe + b'","offset":', None, b',"length":', None,
             b',"uncompressed_length":', None, b"},"]
    n = n_blobs
    cols = [hexed(rng.integers(0, 256, (n, 32), dtype=np.uint8)),
            digits(rng.integers(10_000_000, 99_999_999, n), 8),
            digits(rng.integers(100_000, 999_999, n), 6),
            digits(rng.integers(1_000_000, 9_999_999, n), 7)]
    it = iter(cols)
    row = np.concatenate([np.broadcast_to(np.frombuffer(p, np.uint8), (n, len(p))) if p is not None
                          else next(it) for p in parts], axis=1)
    n_packs = n // per_pack
    head = np.concatenate([
        np.broadcast_to(np.frombuffer(b'{"id":"', np.uint8), (n_packs, 7)),
        hexed(rng.integers(0, 256, (n_packs, 32), dtype=np.uint8)),
        np.broadcast_to(np.frombuffer(b'","blobs":[', np.uint8), (n_packs, 11))], axis=1)
    end = b'],"time":"2024-05-06T07:08:09.123456789+02:00"},'
    tail = np.broadcast_to(np.frombuffer(end, np.uint8), (n_packs, len(end)))
    body = row.reshape(n_packs, -1)[:, :-1]  # no comma after a pack's last blob
    packs = np.concatenate([head, body, tail], axis=1).reshape(-1)[:-1]
    return b'{"packs":[' + packs.tobytes() + b"]}"


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


def upload(texts):
    offs, o = [], 0
    for t in texts:
        offs.append(o)
        o += (len(t) + 15) // 16 * 16
    host = np.zeros(o + 16, np.uint8)
    for a, t in zip(offs, texts):
        host[a:a + len(t)] = np.frombuffer(t, np.uint8)
    return torch.from_numpy(host).to(dev), offs, [len(t) for t in texts]


def main():
    assert torch.cuda.is_available(), "index_load_prof needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; files of {MAX_COUNT} blobs, packs of "
        f"{args.pack_blobs}; reps {args.reps}, warmup {args.warmup}, host reps {args.host_reps}")
    key = Key(bytes(range(64)))
    for lg in [int(x) for x in args.log2.split(",")]:
        rng = np.random.default_rng(lg)
        n_files = -(-(1 << lg) // MAX_COUNT)
        texts = [make_file(rng, MAX_COUNT, args.pack_blobs, tree=(i % 4 == 3)) for i in range(n_files)]
        entries = n_files * MAX_COUNT
        total = sum(len(t) for t in texts)
        sealed = [encrypt_file(key, t, 2) for t in texts]
        say(f"--- 2^{lg}: {n_files} files, {entries} entries, {total / 1e6:.1f} MB of JSON "
            f"({total / entries:.1f} B per blob), {sum(map(len, sealed)) / 1e6:.1f} MB sealed")

        def run(fn):
            dx = DeviceIndex(0)
            fn(dx)
            n = dx.size(DATA) + dx.size(TREE)
            dx.close()
            assert n == entries, n

        rows = []
        if lg <= args.host_log2:
            def host(dx):
                dx.extend(p for t in texts for p in IndexFile.from_json(t).packs)
            rows.append(("host: from_json + extend", clocked(lambda: run(host), args.host_reps, 0)))
        d_json, offs, lens = upload(texts)
        rows.append(("extend_json (text in HBM)",
                     clocked(lambda: run(lambda dx: dx.extend_json(d_json, offs, lens)),
                             args.reps, args.warmup)))
        rows.append(("upload + extend_json",
                     clocked(lambda: run(lambda dx: dx.extend_json(*upload(texts))),
                             args.reps, args.warmup)))
        rows.append(("load (sealed files)",
                     clocked(lambda: run(lambda dx: dx.load(key, sealed)), args.reps, args.warmup)))
        for name, (med, lo, hi) in rows:
            say(f"{name:28s} median {med * 1e3:10.1f} ms  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  "
                f"{entries / med / 1e6:8.2f} M entries/s  {total / med / 1e9:7.3f} GB/s of JSON")
        dx = DeviceIndex(0)
        dx.stage_times = {}
        dx.load(key, sealed)
        say("load, device time by stage (ms): " +
            ", ".join(f"{k} {dx.stage_times.get(k, 0.0):.2f}" for k in ("open", "decode", "parse", "add")))
        dx.close()
        del d_json


if __name__ == "__main__":
    main()
