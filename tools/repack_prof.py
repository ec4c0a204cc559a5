"""Device repack / copy throughput per data kind (repack.BlobCopier): blobs
of 0.5-8 MiB of word text, CSV-like rows and random bytes (the kinds of
tools/zstd_prof.py) are sealed into source "packs" of about --pack-mib with
one key, zstd frames (level 0) or stored, and copied to a second key at level
0 (zstd->zstd, stored->zstd) with BlobCopier.copy, and under the same key
with copy_fast.  Per run: GiB/s of source sealed bytes (and of decoded bytes)
from HIP events around copy + finalize, the host clock around the same work,
and the device time of every stage of that same run -- HIP events around the
calls copy makes (read_partial results into the group buffer, rcdc_aead_open,
rcdc_zstd_decompress, rcdc_zstd_compress, rcdc_aead_seal, the verification
of extra_verify, rcdc_pack_build_raw_multi, rcdc_copy_ranges for the open
pack, the join of the groups' pack buffers, rcdc_sha256_chunks for the pack
ids) -- with their sum and what the
whole run takes beyond it (the host's work between the calls, torch's own
copies).  The source packs are slices of one device buffer
without headers (the copier never reads a header), the blob ids are made up
(the copier carries them, it does not check them); a sample of the new packs
is read back with the destination key and compared with the input."""
import argparse
import hashlib
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from rustic_core_amd import compress, device, pack, read, repack  # noqa: E402
from rustic_core_amd.crypto import Key  # noqa: E402
from rustic_core_amd.index import IndexBlob, Indexer  # noqa: E402
from rustic_core_amd.restore import from_packs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gib", type=float, default=4, help="decoded bytes per run")
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--kinds", default="text,csv,random")
ap.add_argument("--sources", default="zstd,stored")
ap.add_argument("--pack-mib", type=int, default=32, help="source and destination pack size")
ap.add_argument("--batch-mib", type=int, default=1024, help="BlobCopier's batch_bytes")
ap.add_argument("--no-verify", action="store_true", help="extra_verify off")
args = ap.parse_args()
dev = torch.device("cuda:0")
print(f"extra_verify {not args.no_verify}, batch {args.batch_mib} MiB, packs {args.pack_mib} MiB",
      flush=True)
n = int(args.gib * (1 << 30))
rng = np.random.default_rng(1)
lens = []
while sum(lens) < n:
    lens.append(int(rng.integers(512 << 10, 8 << 20)))
lens[-1] -= sum(lens) - n
offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
ids = [hashlib.sha256(b"blob %d" % i).digest() for i in range(len(lens))]
arena = torch.empty(n + 64, dtype=torch.uint8, device=dev)
k_src, k_dst = Key(bytes(range(64))), Key(bytes(range(64, 128)))

words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9))).astype(np.uint8)) for _ in range(400)]
text = np.frombuffer(b" ".join(words[int(i)] for i in rng.integers(0, 400, 16 << 20 >> 2)), np.uint8)
text = torch.from_numpy(text[:16 << 20].copy()).to(dev)
csv_rows = b"".join(b"%08d,%s,%d,%s\n" % (i, words[i % 400], (i * 7919) % 100000, words[(i * 31) % 400])
                    for i in range(600000))
csv_rows = torch.from_numpy(np.frombuffer(csv_rows, np.uint8)[:16 << 20].copy()).to(dev)


def fill(kind):
    if kind == "random":
        arena.random_(0, 256)
    else:
        src = {"text": text, "csv": csv_rows}[kind]
        t = src.numel()
        for o in range(0, n, t):
            arena[o:o + min(t, n - o)] = src[:min(t, n - o)]


class Stages:
    """HIP events around the outermost of the wrapped calls."""

    def __init__(self):
        self.events, self.depth, self.on = [], 0, False

    def wrap(self, name, fn):
        def timed(*a, **k):
            if not self.on or self.depth:
                return fn(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.depth += 1
            try:
                return fn(*a, **k)
            finally:
                self.depth -= 1
                e1.record()
                self.events.append((name, e0, e1))
        return timed

    def take(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.events:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        self.events = []
        return out


stages = Stages()
STAGES = ["load", "open", "decompress", "compress", "seal", "verify", "pack", "carry", "join",
          "pack-id"]
repack.BlobCopier._load = stages.wrap("load", repack.BlobCopier._load)
Key.open_blobs = stages.wrap("open", Key.open_blobs)
read.decompress_frames = stages.wrap("decompress", read.decompress_frames)
compress.compress_blobs = stages.wrap("compress", compress.compress_blobs)
Key.seal_blobs = stages.wrap("seal", Key.seal_blobs)
compress.verify_sealed = stages.wrap("verify", compress.verify_sealed)  # its open_blobs included
repack.build_packs_multi = stages.wrap("pack", repack.build_packs_multi)
repack.copy_ranges = stages.wrap("carry", repack.copy_ranges)
device.sha256_device = stages.wrap("pack-id", device.sha256_device)
torch.cat = stages.wrap("join", torch.cat)  # the groups' pack buffers into one, for the ids


def source(level):
    """The arena's blobs sealed with k_src (frames of ``level``, None:
    stored) and cut into packs; returns (packs, entries, sealed bytes)."""
    sealed, s_offs, s_lens, _, ulens = compress.process_blobs(k_src, arena.data_ptr(), offs, lens, level,
                                                              extra_verify=False)
    packs, entries, first = {}, [], 0
    limit = args.pack_mib << 20
    for i in range(len(lens)):
        end = int(s_offs[i] + s_lens[i])
        if end - int(s_offs[first]) >= limit or i == len(lens) - 1:
            pid = hashlib.sha256(b"pack %d" % len(packs)).digest()
            base = int(s_offs[first])
            packs[pid] = sealed[base:end]
            entries += [(pid, IndexBlob(ids[j], 0, int(s_offs[j]) - base, int(s_lens[j]),
                                        int(ulens[j]) or None)) for j in range(first, i + 1)]
            first = i + 1
    return packs, entries, int(np.asarray(s_lens, np.uint64).sum())


def run(fast, packs, plan, key_dst):
    """One copier over the whole plan; returns (device ms, wall ms, stage
    ms, new packs)."""
    c = repack.BlobCopier(k_src, key_dst, 0, Indexer(lambda f: b"", set()),
                          pack.PackSizer.fixed(args.pack_mib << 20), 0,
                          extra_verify=not args.no_verify, batch_bytes=args.batch_mib << 20)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    stages.on = True
    t0 = time.perf_counter()
    e0.record()
    new = (c.copy_fast if fast else c.copy)(plan, from_packs(packs))
    new += c.finalize()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    stages.on = False
    return e0.elapsed_time(e1), wall, stages.take(), new


def sample_ok(new, key):
    """The first and the last new pack read back and compared with the input."""
    by_id = {b: i for i, b in enumerate(ids)}
    for p in (new[0], new[-1]):
        res = read.read_blobs(key, p.data, p.index.blobs)
        for b, o, ln in zip(p.index.blobs, res.offsets, res.lengths):
            i = by_id[b.id]
            if int(ln) != lens[i] or not torch.equal(res.data[int(o):int(o) + int(ln)],
                                                     arena[int(offs[i]):int(offs[i]) + lens[i]]):
                return False
    return True


with torch.cuda.stream(torch.cuda.Stream(dev)):
    for kind in args.kinds.split(","):
        fill(kind)
        for src_name in args.sources.split(","):
            packs, entries, sealed_bytes = source(0 if src_name == "zstd" else None)
            plan = repack.plan_copy(entries)
            for fast in (False, True):
                key = k_src if fast else k_dst
                runs, best = [], None
                for rep in range(args.reps + 1):  # the first is the warm-up
                    r = run(fast, packs, plan, key)
                    if rep:
                        runs.append(r[:2])
                        if best is None or r[0] < best[0]:
                            best = r  # (the packs of the other runs are dropped)
                    del r
                ms, wall, st, new = best
                out_bytes = sum(int(p.data.numel()) for p in new)
                total = sum(st.values())
                name = f"{src_name}->{src_name} copy_fast" if fast else f"{src_name}->zstd copy"
                print(f"{kind:7s} {name:24s} {len(lens)} blobs in {len(packs)} packs, "
                      f"{len(plan)} reads, {n / 2**30:.1f} GiB decoded, {sealed_bytes / 2**30:.2f} GiB "
                      f"sealed: {' '.join('%.1f' % r[0] for r in runs)} ms (wall "
                      f"{' '.join('%.1f' % r[1] for r in runs)}) = "
                      f"{sealed_bytes / (ms / 1e3) / 2**30:.1f} GiB/s sealed, "
                      f"{n / (ms / 1e3) / 2**30:.1f} GiB/s decoded; {len(new)} new packs, "
                      f"{out_bytes / 2**30:.2f} GiB, sample equals input {sample_ok(new, key)}")
                print(f"{'':7s} stages ms: "
                      + " ".join(f"{s} {st[s]:.1f}" for s in STAGES if s in st)
                      + f" | sum {total:.1f} ms ({total - st.get('pack-id', 0.0):.1f} without pack-id), "
                      f"the run {ms:.1f} ms: {(ms - total) / total * 100:+.0f} % of the sum", flush=True)
                del new, runs, best
            del packs, entries, plan
