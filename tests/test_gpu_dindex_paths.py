"""GPU: a dindex.DeviceIndex where a set or a dict stood -- DeviceIngest's
dedup (ingest.py) and RestorePlan.add_file's index (restore.py) give the
same results with either form of index."""
import hashlib

import numpy as np
import pytest

from oracle import oracle
from rustic_core_amd.errors import ErrorKind, RusticError

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
POLY = oracle.DEFAULT_POLY
KEY = bytes(range(64))


def _batches():
    """Three batches of three streams, a few MiB each: random bytes, zero
    runs (cut at the minimum size: one id many times) and pieces that repeat
    inside a batch and across batches."""
    rng = np.random.default_rng(5)
    rnd = [rng.integers(0, 256, 700 * KiB, dtype=np.uint8).tobytes() for _ in range(5)]
    zeros = bytes(400 * KiB)
    return [
        [rnd[0] + zeros + rnd[1][:300 * KiB], rnd[0], zeros[:100 * KiB] + rnd[2]],
        [rnd[2] + rnd[3], zeros + rnd[1][:300 * KiB], rnd[3][:350 * KiB]],
        [rnd[4] + rnd[0], rnd[4], b"", zeros[:50 * KiB]],
    ]


def _arena(datas):
    import torch
    from rustic_core_amd.device import pack_offsets
    lens = [len(d) for d in datas]
    offs, total = pack_offsets(lens)
    host = np.zeros(total, np.uint8)
    for o, d in zip(offs, datas):
        host[int(o):int(o) + len(d)] = np.frombuffer(d, np.uint8)
    return torch.from_numpy(host).to("cuda:0"), offs, lens


def _run(indexed, batches):
    from rustic_core_amd.chunker import ConfigFile
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.ingest import DeviceIngest
    cfg = ConfigFile(version=2, chunker_polynomial=f"{POLY:x}", chunk_size_=64 * KiB,
                     chunk_min_size_=16 * KiB, chunk_max_size_=256 * KiB,
                     datapack_size=512 * KiB, datapack_growfactor=0)
    ing = DeviceIngest(cfg, Key(KEY), indexed=indexed, long_chunk=128 * KiB)
    out = []
    for k, datas in enumerate(batches):
        arena, offs, lens = _arena(datas)
        res = ing.ingest(arena, offs, lens, finalize=(k == len(batches) - 1))
        packs = [[(b.id, b.offset, b.length, b.uncompressed_length) for b in p.blobs]
                 for p in res.index_packs(pack_ids=[bytes(32)] * len(res.pack_table), time_="t")]
        out.append((res.new.copy(), res.ids.copy(), [np.asarray(c) for c in res.cuts], packs))
    return out


def test_ingest_same_with_set_and_device_index():
    from rustic_core_amd import DeviceIndex
    from rustic_core_amd.dindex import DATA
    batches = _batches()
    # what a first, index-less run stores; half of it is "already in the repository"
    first = _run(set(), batches[:1])
    ids0 = [bytes(i) for i in first[0][1]]
    known = set(ids0[::2])
    assert 0 < len(known) < len(set(ids0))
    the_set = set(known)
    dx = DeviceIndex(0)
    dx.add_ids(np.frombuffer(b"".join(sorted(known)), np.uint8).reshape(-1, 32))
    a = _run(the_set, batches)
    b = _run(dx, batches)
    n_new = 0
    for (new_a, ids_a, cuts_a, packs_a), (new_b, ids_b, cuts_b, packs_b) in zip(a, b):
        assert np.array_equal(ids_a, ids_b)
        assert len(cuts_a) == len(cuts_b) and all(np.array_equal(x, y)
                                                  for x, y in zip(cuts_a, cuts_b))
        assert new_a.tolist() == new_b.tolist()
        assert packs_a == packs_b
        n_new += int(new_a.sum())
    every = [bytes(i) for r in a for i in r[1]]
    # the batches had repeats inside and across, long and short chunks, and packs
    assert n_new < len(set(every)) < len(every)
    lens = np.concatenate([np.diff(np.concatenate([[0], c])) for r in a for c in r[2] if len(c)])
    assert (lens > 128 * KiB).any() and (lens <= 128 * KiB).any()
    assert sum(len(r[3]) for r in a) >= 3
    # the device index now has exactly what the set has
    assert the_set == known | set(every)
    assert dx.keys(DATA) == len(the_set) and dx.size(DATA) == len(the_set)
    q = sorted(the_set) + [hashlib.sha256(b"absent %d" % k).digest() for k in range(50)]
    has = dx.has(DATA, np.frombuffer(b"".join(q), np.uint8).reshape(-1, 32)).cpu().tolist()
    assert has == [i in the_set for i in q]
    dx.close()


def test_ingest_refuses_an_index_on_another_device():
    from rustic_core_amd import DeviceIndex
    from rustic_core_amd.chunker import ConfigFile
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.ingest import DeviceIngest
    with pytest.raises(RusticError) as e:
        DeviceIngest(ConfigFile.new(2, POLY), Key(KEY), device=0, indexed=DeviceIndex(1))
    assert e.value.kind == ErrorKind.InvalidInput


def test_restore_plan_same_with_dict_and_device_index():
    import torch
    from rustic_core_amd import DeviceIndex, RestorePlan, index_lookup
    from rustic_core_amd.index import IndexBlob, IndexFile, IndexPack
    rng = np.random.default_rng(9)
    chunks = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (5000, 70, 9000, 1234)]
    ids = [hashlib.sha256(c).digest() for c in chunks]
    P1, P2, P3 = (hashlib.sha256(b"pack %d" % k).digest() for k in range(3))
    gone = hashlib.sha256(b"only in packs_to_delete").digest()
    f1 = IndexFile([IndexPack(P1, [IndexBlob(ids[0], 0, 0, 2100, 5000),
                                   IndexBlob(ids[1], 0, 2100, 70 + 32, None),   # no uncompressed
                                   IndexBlob(ids[2], 0, 2202, 4000, 9000)])],
                   [IndexPack(P3, [IndexBlob(gone, 0, 0, 77, None)])])
    f2 = IndexFile([IndexPack(P2, [IndexBlob(ids[0], 0, 40, 2222, 5000),        # an id in two packs
                                   IndexBlob(ids[3], 0, 2262, 800, 1234)])])
    files = [f1, f2]
    as_dict = index_lookup(files)
    dx = DeviceIndex.from_index_files(files)
    file_a = [0, 1, 2, 0, 3]
    file_b = [3, 1]
    data_a = b"".join(chunks[k] for k in file_a)
    damaged = bytearray(data_a)
    damaged[5000 + 70 + 17] ^= 1          # inside the third blob of file a
    plans = []
    for index in (as_dict, dx):
        plan = RestorePlan()
        r = [plan.add_file("a", len(data_a), [ids[k] for k in file_a], index,
                           existing=bytes(damaged)),
             plan.add_file("b", 1304, [ids[k] for k in file_b], index),
             plan.add_file("c", len(data_a), [ids[k] for k in file_a], index,
                           existing=bytes(data_a)),
             plan.add_file("empty", 0, [], index)]
        with pytest.raises(RusticError) as e:
            plan.add_file("d", 77, [ids[1], gone], index)
        assert e.value.kind == ErrorKind.Internal
        assert e.value.message == f"Blob ID `{gone.hex()}` not found in index, but should be there."
        plans.append((plan, r))
    (pa, ra), (pb, rb) = plans
    assert ra == rb == ["Modify", "Modify", "Verified", "Modify"]
    assert pa.restore_info() == pb.restore_info()
    assert pa.names == pb.names == ["a", "b", "c", "empty"]
    assert pa.file_lengths == pb.file_lengths == [len(data_a), 1304, len(data_a), 0]
    assert (pa.restore_size, pa.matched_size) == (pb.restore_size, pb.matched_size)
    assert pa.restore_size == 9000 + 1304 and pa.matched_size == 2 * len(data_a) - 9000
    assert [(r.pack_id, r.from_file, r.offset, r.length, r.blobs) for r in pa.pack_reads()] == \
        [(r.pack_id, r.from_file, r.offset, r.length, r.blobs) for r in pb.pack_reads()]
    # the first entry of the id that is in two packs wins, in both
    assert (P1, 0, 2100, 5000) in pb.r and not any(k[0] == P2 and k[1] == 40 for k in pb.r)
    assert (P1, 2100, 102, 0) in pb.r
    assert sorted(pb.existing) == [0, 2]
    assert all(isinstance(t, torch.Tensor) for t in pb.existing.values())
    dx.close()
