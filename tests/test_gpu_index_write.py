"""Index files written on the device (rcdc_index_write, save_index_files,
DeviceIndexer, PrunePlan.write_index).  The expected bytes everywhere are
``IndexFile.to_json()`` of the same content -- today's host path."""
import hashlib
import random

import numpy as np
import pytest

from tests.index_json_cases import random_index

pytestmark = pytest.mark.gpu

GUARD = 4096
T1 = "2024-05-06T07:08:09.123456789+02:00"
# 0, then both sides of every digit-count boundary of a u32
EDGES = [0] + [v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k)] + [4294967295]


def _id(n: int) -> bytes:
    return hashlib.sha256(b"ixw%d" % n).digest()


def _uniform(f):
    """``f`` with every blob given the type of its pack's first blob."""
    for p in f.packs + f.packs_to_delete:
        for b in p.blobs:
            b.type = p.blobs[0].type
    return f


def _records(files):
    """Entry arrays (numpy), PackRecords and FileRecords of IndexFiles whose
    packs hold blobs of one type each."""
    from rustic_core_amd.index_write import FileRecord, PackRecord
    ids, ints, packs, frecs = [], [], [], []
    for f in files:
        first = len(packs)
        for p in list(f.packs) + list(f.packs_to_delete):
            assert len({b.type for b in p.blobs}) <= 1
            packs.append(PackRecord(p.id, p.blobs[0].type if p.blobs else 0, len(ids),
                                    len(p.blobs), p.time, p.size))
            for b in p.blobs:
                ids.append(b.id)
                ints.append((b.offset, b.length, b.uncompressed_length or 0))
        frecs.append(FileRecord(first, len(packs) - first, len(f.packs_to_delete), f.supersedes))
    a_ids = np.frombuffer(b"".join(ids), np.uint8).reshape(len(ids), 32)
    a = np.array(ints, np.uint32).reshape(len(ints), 3)
    return (a_ids, a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()), packs, frecs


def _check_written(w, want):
    """``w`` holds exactly the texts ``want``: every file byte-equal, at
    16-byte aligned offsets in order, and nothing else of the allocation
    written (0xA5 in the gaps, behind the last file and in the guard)."""
    assert len(w) == len(want)
    raw = w.raw.cpu().numpy()
    assert len(raw) >= w.cap + GUARD
    covered = np.zeros(len(raw), bool)
    end = 0
    for i, text in enumerate(want):
        o, n = int(w.offs[i]), int(w.lens[i])
        assert o % 16 == 0 and o == (end + 15) // 16 * 16, i
        got = raw[o:o + n].tobytes()
        assert n == len(text) and got == text, (i, got[:200], text[:200])
        covered[o:o + n] = True
        end = o + n
    assert w.total == end <= w.cap
    assert (raw[~covered] == 0xA5).all()


def _write(files, **kw):
    from rustic_core_amd.index_write import write_json
    arrays, packs, frecs = _records(files)
    w = write_json(*arrays, packs, frecs, guard=GUARD, **kw)
    _check_written(w, [f.to_json() for f in files])
    return w


def _pack(seed, n_blobs, tpe=0, time=None, size=None, ints=None):
    from rustic_core_amd.index import IndexPack
    p = IndexPack(_id(seed), time=time, size=size)
    for j in range(n_blobs):
        off, ln, ul = ints[j] if ints else ((seed * 131 + j * 977) % (1 << 20), 10 ** (j % 10),
                                            (j % 4) and 7 ** (j % 11))
        p.add(_id(seed * 1000 + j), tpe, off, ln, ul or None)
    return p


def _case_table():
    from rustic_core_amd.index import IndexFile
    c = []
    c.append(("empty", IndexFile()))
    c.append(("supersedes_none", IndexFile(packs=[_pack(1, 2)])))
    c.append(("supersedes_empty", IndexFile(packs=[_pack(2, 1)], supersedes=[])))
    c.append(("supersedes_two", IndexFile(packs=[_pack(3, 3, 1)], supersedes=[_id(90), _id(91)])))
    c.append(("supersedes_only", IndexFile(supersedes=[_id(92)])))
    c.append(("delete_only", IndexFile(packs_to_delete=[_pack(4, 2, 1, T1), _pack(5, 0)])))
    c.append(("packs_and_delete", IndexFile(packs=[_pack(6, 2), _pack(7, 1, 1)],
                                            packs_to_delete=[_pack(8, 3, 0, T1, 77)],
                                            supersedes=[_id(93)])))
    c.append(("pack_without_blobs", IndexFile(packs=[_pack(9, 0), _pack(10, 0, 1, T1),
                                                      _pack(11, 0, 0, None, 0), _pack(12, 1)])))
    for k, (time, size) in enumerate(((None, None), (T1, None), (None, 4294967295), ("", 12345),
                                      ("{[ ]},:~ ", 9))):
        c.append((f"time_size_{k}", IndexFile(packs=[_pack(20 + k, 2, k % 2, time, size)])))
    c.append(("ulen_null", IndexFile(packs=[_pack(30, 3, 0, ints=[(0, 0, 0), (5, 6, 0), (1, 2, 3)])])))
    for which in range(3):  # offset, length, uncompressed length through every edge
        ints = [tuple(v if k == which else 5 for k in range(3)) for v in EDGES]
        c.append((f"digits_{which}", IndexFile(packs=[_pack(40 + which, len(ints), which % 2,
                                                           ints=ints)])))
    c.append(("all_max", IndexFile(packs=[_pack(50, 3, 1, ints=[(4294967295,) * 3] * 3)])))
    return c


def test_case_table(gpu_ctx):
    cases = _case_table()
    assert cases[0][1].to_json() == b'{"packs":[]}'
    assert b'"supersedes":[],' in cases[2][1].to_json()
    assert b"packs_to_delete" not in cases[1][1].to_json()
    assert b'"uncompressed_length":null' in dict(cases)["ulen_null"].to_json()
    for name, f in cases:
        _write([f])
    _write([f for _, f in cases])


MAX_SHIFT = 3 * 85 + 64 + 27


def _shifted(s, body):
    """A file whose ``body`` packs begin ``s`` bytes later than at s == 0:
    0 .. 3 packs without blobs (85 bytes each), a time of 0 .. 64 bytes and
    0 .. 27 more digits in the first pack's blob."""
    from rustic_core_amd.index import IndexFile
    assert 0 <= s <= MAX_SHIFT
    j = min(s // 85, 3)
    s -= 85 * j
    t = min(s, 64)
    s -= t
    d = [min(s, 9), min(max(s - 9, 0), 9), min(max(s - 18, 0), 9)]
    lead = _pack(7000, 1, 0, "x" * t, ints=[tuple(10 ** k for k in d)])
    return IndexFile(packs=[lead] + [_pack(7001 + i, 0) for i in range(j)] + body)


def _edge_distances(text, span):
    """For every span boundary inside ``text`` (the file lies at offset 0):
    how far behind the start of its blob object or pack head it falls."""
    blobs, heads = set(), set()
    for b in range(span, len(text), span):
        start = text.rfind(b'{"id":"', 0, b + 7)
        if start < 0:
            continue
        if text[start + 71:start + 79] == b'","type"':
            end = text.index(b"}", start) + 1
            if b < end:
                blobs.add(b - start)
        elif b - start < 82:
            heads.add(b - start)
    return blobs, heads


def _most_in_a_span(text, span, marker, width):
    """The most pieces of ``text`` (beginning with ``marker``, ``width`` bytes
    long at least) that one span of the output touches."""
    starts, at = [], text.find(marker)
    while at >= 0:
        starts.append(at)
        at = text.find(marker, at + 1)
    starts = np.array(starts)
    return max(int(((starts < s + span) & (starts + width > s)).sum()) for s in range(0, len(text), span))


def test_more_than_64_pieces_in_a_span(gpu_ctx):
    """The wave that writes a span takes the span's pack heads and its files
    64 at a time, one a lane: packs without blobs and empty files, so that a
    span holds more than 64 of each and both loops take a second pass.  (The
    loop over blob objects never does: the smallest is 134 bytes long, and a
    span touches 62 of those at the most, which is asserted here.)"""
    from rustic_core_amd.index import IndexFile
    from rustic_core_amd.index_write import write_span
    span = write_span()
    blobs = IndexFile(packs=[_pack(900, 300, ints=[(j % 10, 1, 1) for j in range(300)])])
    assert 60 <= _most_in_a_span(blobs.to_json(), span, b'","type"', 50) <= 64
    packs = IndexFile(packs=[_pack(1000 + i, 0, i % 2) for i in range(300)])
    assert _most_in_a_span(packs.to_json(), span, b'{"id":"', 80) > 64
    for f in (blobs, packs):
        assert len(f.to_json()) > 2 * span
        _write([f])
    empty = [IndexFile(), IndexFile(packs=[_pack(2000, 0)])] * 150
    assert span // 112 > 64 and all(len(f.to_json()) <= 112 for f in empty)
    _write(empty)
    _write([blobs] + empty + [packs])


def test_lane_wave_and_span_edges(gpu_ctx):
    from rustic_core_amd.index import IndexFile
    from rustic_core_amd.index_write import write_span
    span = write_span()
    assert span % 16 == 0 and span >= 1024
    # packs around the wave's 64 lanes, in one file and one file each
    sizes = (1, 63, 64, 65, 127, 128, 129, 257)
    packs = [_pack(100 + i, n, i % 2, T1 if i % 3 == 0 else None) for i, n in enumerate(sizes)]
    _write([IndexFile(packs=packs)] + [IndexFile(packs=[p]) for p in packs])
    # more files than a wave has lanes
    many = [IndexFile(packs=[_pack(300 + i, i % 4, i % 2)]) for i in range(70)]
    assert len(many) > 64  # a second round of the wave that places the files, with its carry
    _write(many)
    # a file of about three spans behind every shift up to the longest object:
    # every byte of a blob object and of a pack head meets a span edge
    body = [_pack(500 + i, 1 + i % 7, i % 2, T1 if i % 2 else None, i * 1001 if i % 3 == 0 else None)
            for i in range(3 * span // 600)]
    blobs, heads = set(), set()
    files = [_shifted(s, body) for s in range(MAX_SHIFT + 1)]
    base = len(files[0].to_json())
    for s, f in enumerate(files):
        text = f.to_json()
        assert len(text) == base + s and 2 * span < len(text) < 5 * span
        b, h = _edge_distances(text, span)
        blobs |= b
        heads |= h
    assert blobs >= set(range(133)) and heads >= set(range(82))
    for f in files:
        _write([f])
    _write(files[::13])


def test_nothing_else_is_written(gpu_ctx):
    """Files whose lengths run through every residue of 16, so every size of
    ragged end and of gap occurs; the check is _check_written's."""
    from rustic_core_amd.index import IndexFile
    files = [IndexFile(packs=[_pack(900 + k, 1, 0, "t" * k)]) for k in range(33)]
    assert {len(f.to_json()) % 16 for f in files} == set(range(16))
    w = _write(files)
    assert all(int(o) % 16 == 0 for o in w.offs)
    assert w.total < w.cap


def _parse(texts):
    from rustic_core_amd.dindex import PARSED, parse_json
    from tests.test_gpu_index_parse import _arena
    d, offs, lens = _arena(texts, 16)
    res = parse_json(d, offs, lens)
    assert res.files["status"].tolist() == [PARSED] * len(texts)
    return res


def test_strides(gpu_ctx):
    import torch
    from rustic_core_amd.index import IndexFile
    from rustic_core_amd.index_write import write_json
    files = [IndexFile(packs=[_pack(1100 + 10 * i + j, 1 + (i + j) % 9) for j in range(4)])
             for i in range(3)]
    want = [f.to_json() for f in files]
    res = _parse(want)
    n = res.entries[0]
    ids, locs = res.ids[0], res.locs[0]
    assert locs.stride(0) == 4 and locs[:, 1].stride(0) == 4  # 16 bytes
    arrays, packs, frecs = _records(files)
    assert n == len(arrays[0]) and res.entries[1] == 0
    a = write_json(ids, locs[:, 1], locs[:, 2], locs[:, 3], packs, frecs, guard=GUARD)
    _check_written(a, want)
    b = write_json(ids[:n].clone(), locs[:n, 1].contiguous(), locs[:n, 2].contiguous(),
                   locs[:n, 3].contiguous(), packs, frecs, guard=GUARD)
    _check_written(b, want)
    assert torch.equal(a.data, b.data)
    # ids in rows of 48 bytes that start 1 byte off a word: read byte by byte
    wide = torch.zeros((n, 48), dtype=torch.uint8, device="cuda:0")
    wide[:, 1:33] = ids[:n]
    c = write_json(wide[:, 1:33], locs[:n, 1], locs[:n, 2], locs[:n, 3], packs, frecs, guard=GUARD)
    _check_written(c, want)


def test_parse_then_write_is_the_identity(gpu_ctx):
    import torch
    from rustic_core_amd.index import IndexFile
    from rustic_core_amd.index_write import FileRecord, PackRecord, write_json
    rng = random.Random(31)
    files = []
    for _ in range(20):
        f = _uniform(random_index(rng, rng.randrange(1, 9), 70))
        for p in f.packs + f.packs_to_delete:
            p.time = p.size = None
        files.append(IndexFile(packs=f.packs + f.packs_to_delete))
    texts = [f.to_json() for f in files]
    res = _parse(texts)
    e = res.entries
    assert e[0] > 300 and e[1] > 300
    ids = torch.cat([res.ids[t][:e[t]] for t in (0, 1)])
    locs = torch.cat([res.locs[t][:e[t]] for t in (0, 1)])
    counts = [len(p.blobs) for f in files for p in f.packs]
    first = [0, e[0]]
    packs = []
    for p, c in zip(res.packs, counts):
        t = int(p["type"])
        packs.append(PackRecord(p["id"].tobytes(), t, first[t], c))
        first[t] += c
    assert first == [e[0], e[0] + e[1]]
    frecs, k = [], 0
    for f in res.files:
        frecs.append(FileRecord(k, int(f["packs"].sum())))
        k += int(f["packs"].sum())
    w = write_json(ids, locs[:, 1], locs[:, 2], locs[:, 3], packs, frecs, guard=GUARD)
    _check_written(w, texts)


def _saved(key, ids, sealed, offs, lens, version):
    """The sealed files on the host, their ids checked, and their texts."""
    from rustic_core_amd.compress import decode_all
    h = sealed.cpu().numpy()
    out, texts = [], []
    for i, (o, n) in enumerate(zip(offs, lens)):
        s = h[int(o):int(o) + int(n)].tobytes()
        assert ids[i] == hashlib.sha256(s).digest(), i
        plain = key.decrypt_data(s)
        if version >= 2:
            assert plain[0] == 2
            plain = decode_all(plain[1:])
        out.append(s)
        texts.append(plain)
    return out, texts


@pytest.mark.parametrize("version", [2, 1])
def test_write_then_load(gpu_ctx, version):
    from rustic_core_amd import DeviceIndex
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.dindex import PARSED
    from rustic_core_amd.index_write import save_index_files
    from tests.test_gpu_index_parse import _same_index
    rng = random.Random(47 + version)
    key = Key(bytes(range(64)))
    files = [_uniform(random_index(rng, 8, 60)) for _ in range(5)]
    w = _write(files)
    ids, sealed, offs, lens = save_index_files(key, w, version=version)
    assert len(ids) == len(files) and all(int(o) % 16 == 0 for o in offs)
    blobs, texts = _saved(key, ids, sealed, offs, lens, version)
    assert texts == [f.to_json() for f in files]
    dx = DeviceIndex(0)
    assert dx.load(key, blobs).tolist() == [PARSED] * len(files)
    _same_index(dx, files)
    dx.close()
    # given nonces are used, and no file saves nothing
    nonces = [bytes([i]) * 16 for i in range(len(files))]
    ids2, sealed2, offs2, lens2 = save_index_files(key, w, version=version, nonces=nonces)
    h = sealed2.cpu().numpy()
    assert [h[int(o):int(o) + 16].tobytes() for o in offs2] == nonces
    assert save_index_files(key, _write([]), version=version)[0] == []


def test_device_indexer_end_to_end(gpu_ctx, monkeypatch):
    import torch
    from rustic_core_amd import index
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.index_write import DeviceIndexer, PackRecord
    key = Key(bytes(range(64)))
    packs = [_pack(2000 + i, (i * 37) % 120, i % 2, T1 if i % 3 else None) for i in range(85)]
    assert 4500 < sum(len(p.blobs) for p in packs) < 5500
    deletes = [i % 7 == 3 for i in range(len(packs))]
    # the yardstick: index.Indexer at the same limit
    monkeypatch.setattr(index, "MAX_COUNT", 1000)
    want = []
    host = index.Indexer(lambda f: want.append(f.to_json()) or b"")
    for p, d in zip(packs, deletes):
        host.add(p, d)
    host.finalize()
    assert len(want) >= 5
    # every other pack as a record into device arrays, the rest as host packs
    dev_packs = [p for i, p in enumerate(packs) if i % 2 == 0]
    (a_ids, a_off, a_len, a_ul), recs, _ = _records([index.IndexFile(packs=dev_packs)])
    up = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).to("cuda:0")
    entries = (up(a_ids), up(a_off), up(a_len), up(a_ul))
    for flush_files in (None, 2):
        got, saved = [], []

        def save(ids, sealed, offs, lens):
            got.extend(_saved(key, ids, sealed, offs, lens, 2)[1])
            saved.extend(ids)
        ix = DeviceIndexer(save, max_count=1000, key=key, entries=entries, flush_files=flush_files)
        k = 0
        for i, (p, d) in enumerate(zip(packs, deletes)):
            if i % 2 == 0:
                ix.add(recs[k], d)
                k += 1
            else:
                ix.add(p, d)
        if flush_files:
            assert len(got) >= 2  # saved before finalize
        ix.finalize()
        assert got == want and ix.saved == saved
    # an empty finalize saves nothing
    ix = DeviceIndexer(lambda *a: got.append(None), max_count=1000, key=key)
    ix.finalize()
    assert got == want


def test_prune_write_index(gpu_ctx):
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.index import IndexBlob, IndexFile, IndexPack
    import torch
    from rustic_core_amd.prune import PackToDo, PruneOptions, PrunePack, PrunePlan
    from tests.prune_cases import (CONFIG, NOW, OLD, YOUNG, bid, existing_of, ids_array, one_file,
                                   pack, plan_of, plan_summary)
    key = Key(bytes(range(64)))
    files = [
        one_file([pack("k1", [("a", 10), ("b", 20)], time=OLD), pack("r1", [("c", 10), ("x", 20)]),
                  pack("d1", [("y", 5)], time=OLD), pack("k2", [("d", 7)], tpe=1)],
                 [pack("m1", [("z", 9)], time=YOUNG), pack("rec", [("e", 3), ("q", 4)], time=OLD)]),
        one_file([pack("k3", [("f", 1), ("g", 2), ("h", 3)]), pack("r2", [("i", 6), ("w", 8)], tpe=1),
                  pack("d2", [("v", 2)]), pack("k4", [("j", 2)], time=YOUNG)],
                 [pack("m2", [("u", 1)], time=YOUNG), pack("m3", [("t", 1)])]),
    ]
    used = list("abcdefghij")
    opts = PruneOptions(max_unused="0%", max_repack="unlimited", no_resize=True)
    # the entries as device tensors, one PrunePack record per pack (from_entries)
    recs, b_ids, b_ints = [], [], []
    for fno, f in enumerate(files):
        for marked, packs in ((False, f.packs), (True, f.packs_to_delete)):
            for p in packs:
                recs.append(PrunePack(p.id, p.blobs[0].type, p.pack_size(), p.time, marked, fno,
                                      len(b_ids), len(p.blobs)))
                b_ids += [b.id for b in p.blobs]
                b_ints += [(b.offset, b.length, b.uncompressed_length or 0) for b in p.blobs]
    d_ids = torch.from_numpy(np.frombuffer(b"".join(b_ids), np.uint8).reshape(-1, 32).copy()).to("cuda:0")
    d_ints = torch.from_numpy(np.array(b_ints, np.int32)).to("cuda:0")  # columns: strided views
    pairs = [(bid("index:%d" % i), f) for i, f in enumerate(files)]
    plan = PrunePlan.from_entries(d_ids, d_ints[:, 1], d_ints[:, 2], d_ints[:, 0], recs,
                                  [i for i, _ in pairs], torch.from_numpy(ids_array(used)).to("cuda:0"),
                                  existing_of(pairs), opts, CONFIG, NOW, device=0)
    assert plan_summary(plan) == plan_summary(plan_of(files, used, device=None, opts=opts))
    todo = {p.to_do for p in plan.packs}
    assert len(plan.packs) == 12
    assert todo >= {PackToDo.Keep, PackToDo.Repack, PackToDo.MarkDelete, PackToDo.KeepMarked,
                    PackToDo.Recover}
    assert len(plan.index_files) == 2
    now = "2024-05-01T12:00:00+00:00"
    got = []
    ix = plan.write_index(key, prune_time=now, max_count=12,
                          save=lambda ids, sealed, offs, lens: got.extend(
                              _saved(key, ids, sealed, offs, lens, 2)[1]))
    assert got == []  # not finalized
    ix.finalize()
    # the same files from index_updates, built on the host
    ids, offs, lens, ulens = (plan._host(a) for a in (plan._ids, plan._offsets, plan._lens,
                                                       plan._ulens))
    want, f, count = [], IndexFile(), 0
    for rec, delete in plan.index_updates(now, False).adds:
        p = IndexPack(rec.id, time=rec.time, size=rec.size)
        for e in range(rec.first, rec.first + rec.count):
            p.blobs.append(IndexBlob(ids[e].tobytes(), rec.type, int(offs[e]), int(lens[e]),
                                     int(ulens[e]) or None))
        f.add(p, delete)
        count += rec.count
        if count >= 12:
            want.append(f.to_json())
            f, count = IndexFile(), 0
    if f.packs or f.packs_to_delete:
        want.append(f.to_json())
    assert len(want) >= 2 and got == want
