"""CPU: rcdc_index_write's ABI without a device (symbols, structs, the bound,
what is refused before any HIP call), PrunePlan.index_updates on the host
engine, and DeviceIndexer's split rule against index.Indexer."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from tests.index_json_cases import random_index

SYMBOLS = ("rcdc_index_write", "rcdc_index_write_bound", "rcdc_index_write_span")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 4294967295


def test_symbols_and_structs(rcdc_lib):
    from rustic_core_amd import _lib
    from rustic_core_amd.index_write import (HAS_SIZE, HAS_TIME, IXW_FILE, IXW_OUT, IXW_PACK,
                                             MAX_TIME, write_span)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    header = open(os.path.join(ROOT, "include", "rcdc.h")).read()
    for ct, dt, name, size in ((_lib.IxwritePack, IXW_PACK, "rcdc_ixwrite_pack", 64),
                               (_lib.IxwriteFile, IXW_FILE, "rcdc_ixwrite_file", 32),
                               (_lib.IxwriteOut, IXW_OUT, "rcdc_ixwrite_out", 16)):
        assert ctypes.sizeof(ct) == dt.itemsize == size
        assert [f[0] for f in ct._fields_] == list(dt.names)
        assert [getattr(ct, f[0]).offset for f in ct._fields_] == [dt.fields[n][1] for n in dt.names]
        assert re.search(r"\}\s*%s;\s*/\*\s*%d B\s*\*/" % (name, size), header), name
    defs = dict(re.findall(r"#define (RCDC_IXWRITE_\w+)\s+(\d+)u", header))
    assert int(defs["RCDC_IXWRITE_SPAN"]) == write_span() == rcdc_lib.rcdc_index_write_span()
    assert int(defs["RCDC_IXWRITE_MAX_TIME"]) == MAX_TIME
    assert (int(defs["RCDC_IXWRITE_HAS_TIME"]), int(defs["RCDC_IXWRITE_HAS_SIZE"])) == \
        (HAS_TIME, HAS_SIZE)
    assert write_span() % 16 == 0 and write_span() >= 1024
    assert rcdc_lib.rcdc_abi_version() == 5 and "#define RCDC_ABI_VERSION 5u" in header


def _counts(f):
    packs = f.packs + f.packs_to_delete
    return (sum(len(p.blobs) for p in packs), len(packs), 1, len(f.supersedes or ()),
            sum(len(p.time) for p in packs if p.time is not None))


def test_bound_against_the_largest_objects(rcdc_lib):
    from rustic_core_amd.index import IndexFile, IndexPack
    from rustic_core_amd.index_write import MAX_TIME, write_bound
    assert write_bound(0, 0, 0) == 0

    def big_pack(n):
        p = IndexPack(bytes([0xFF]) * 32, time="9" * MAX_TIME, size=U32)
        for _ in range(n):
            p.add(bytes([0xEE]) * 32, 0, U32, U32, U32)
        return p
    blob = big_pack(1).blobs[0].to_obj()
    from tests.index_json_cases import compact
    assert len(compact(blob)) == 160 and len(IndexPack(bytes(32)).to_obj()["id"]) == 64
    assert len(compact(IndexPack(bytes(32)).to_obj())) == 84
    for n_blobs, n_packs, n_del, n_sup in ((1, 1, 0, 0), (3, 2, 2, 2), (50, 7, 3, 1), (0, 4, 4, 0),
                                           (0, 0, 0, 5), (200, 1, 0, 0)):
        f = IndexFile(packs=[big_pack(n_blobs) for _ in range(n_packs)],
                      packs_to_delete=[big_pack(n_blobs) for _ in range(n_del)],
                      supersedes=[bytes([0xAB]) * 32] * n_sup)
        text = f.to_json()
        bound = write_bound(*_counts(f))
        assert bound >= len(text) + 15, (n_blobs, n_packs, n_del, n_sup)
        # and it is tight for these: only the commas no first element has,
        # a root key not written and the padding are slack
        assert bound - len(text) <= 15 + 49 + 2 + n_packs + n_del


def test_bound_over_random_files(rcdc_lib):
    from rustic_core_amd.index_write import write_bound
    rng = random.Random(20241020)
    total = 0
    for k in range(40):
        f = random_index(rng, rng.randrange(8), 30)
        assert write_bound(*_counts(f)) >= len(f.to_json()) + 15, k
        total += (len(f.to_json()) + 15) // 16 * 16
    assert total > 50_000  # the files are not trivial


def test_refused_before_any_hip_call(rcdc_lib):
    """Every refusal is InvalidInput (2) with its message and no device: the
    context and the device pointers are dummies that are never read."""
    from rustic_core_amd import _lib
    L = rcdc_lib
    fake = ctypes.c_void_p(64)   # a context / 16-byte aligned device memory
    packs = (_lib.IxwritePack * 2)()
    files = (_lib.IxwriteFile * 1)()
    out = (_lib.IxwriteOut * 1)()
    sup = (ctypes.c_uint8 * 64)()
    times = ctypes.create_string_buffer(b"2024-01-02T03:04:05Z", 20)
    total = ctypes.c_uint64(7)

    def reset():
        for p in packs:
            p.first, p.count, p.type, p.flags, p.size, p.time_off, p.time_len = 0, 4, 0, 0, 0, 0, 0
        packs[1].flags, packs[1].time_len = 1, 20
        f = files[0]
        f.pack_first, f.pack_count, f.n_delete = 0, 2, 1
        f.sup_first, f.sup_count, f.has_supersedes = 0, 2, 1
    reset()
    big = 1 << 20
    A = ctypes.addressof

    def call(ctx=fake, ids=fake, id_stride=32, off=fake, off_stride=4, ln=fake, len_stride=16,
             ul=fake, ul_stride=4, n=8, packs_=A(packs), n_packs=2, files_=A(files), n_files=1,
             sup_=A(sup), n_sup=2, times_=A(times), tb=20, d_out=fake, cap=big, out_=A(out),
             total_=ctypes.byref(total)):
        total.value = 7
        return L.rcdc_index_write(ctx, ids, id_stride, off, off_stride, ln, len_stride, ul,
                                  ul_stride, n, packs_, n_packs, files_, n_files, sup_, n_sup,
                                  times_, tb, d_out, cap, out_, total_, None)

    def refused(message, **kw):
        assert call(**kw) == 2, kw
        assert message in _lib.last_error(), (kw, _lib.last_error())
        assert total.value == 7  # nothing written
    refused("ctx is NULL", ctx=None)
    refused("total is NULL", total_=None)
    for kw in ({"ids": None}, {"off": None}, {"ln": None}, {"ul": None}, {"packs_": None},
               {"files_": None}, {"sup_": None}, {"times_": None}, {"d_out": None}, {"out_": None}):
        refused("null array", **kw)
    # ranges past the arrays
    refused("entries lie outside", n=3)
    packs[0].first = 2 ** 64 - 1
    refused("entries lie outside")
    reset()
    refused("packs lie outside", n_packs=1)
    files[0].pack_first = 2 ** 64 - 2
    refused("packs lie outside")
    reset()
    refused("supersedes lie outside", n_sup=1)
    refused("time lies outside", tb=19)
    files[0].n_delete = 3
    refused("n_delete above pack_count")
    reset()
    # alignment
    for kw in ({"off": ctypes.c_void_p(66)}, {"ln": ctypes.c_void_p(65)}, {"ul": ctypes.c_void_p(67)},
               {"off_stride": 6}, {"len_stride": 1}, {"ul_stride": 18}):
        refused("4-byte aligned", **kw)
    refused("16-byte aligned", d_out=ctypes.c_void_p(72))
    # types, flags, times
    packs[1].type = 2
    refused("type is above 1")
    reset()
    packs[0].flags = 4
    refused("unknown pack flags")
    reset()
    for bad in (b'"', b"\\", b"\x1f", b"\x7f", b"\xc3", b"\n", b"\x00"):
        times.raw = b"2024-01-02T" + bad + b"3:04:05Z"
        refused("a time holds a byte outside", tb=20)
    times.raw = b"2024-01-02T03:04:05Z"
    packs[1].time_len = 65
    long_times = ctypes.create_string_buffer(b"1" * 65, 65)
    refused("longer than RCDC_IXWRITE_MAX_TIME", times_=A(long_times), tb=65)
    reset()
    # a time that is not written is not looked at
    packs[1].flags = 0
    times.raw = b'"' * 20
    bound = L.rcdc_index_write_bound(8, 2, 1, 2, 0)
    refused("cap_out below", cap=bound - 1)
    times.raw = b"2024-01-02T03:04:05Z"
    reset()
    # the capacity: the written counts decide (one range written twice counts twice)
    bound = L.rcdc_index_write_bound(8, 2, 1, 2, 20)
    assert bound == 161 * 8 + 113 * 2 + 20 + 67 * 2 + 64
    refused("cap_out below", cap=bound - 1)
    refused("cap_out below", cap=0)
    # n_files == 0 launches nothing: fine without arrays (the context is not touched)
    assert L.rcdc_index_write(fake, None, 32, None, 4, None, 4, None, 4, 0, None, 0, None, 0, None,
                              0, None, 0, None, 0, None, ctypes.byref(total), None) == 0
    assert total.value == 0


def test_python_argument_checks():
    from rustic_core_amd.errors import RusticError
    from rustic_core_amd.index_write import (FileRecord, PackRecord, file_records, pack_records)
    recs, times = pack_records([PackRecord(bytes(32), 1, 5, 6, "ab", 7),
                                PackRecord(bytes(32), 0, 0, 0, "ab"), (bytes(32), 0, 1, 2)])
    assert times == b"ab" and recs["flags"].tolist() == [3, 1, 0]
    assert recs["time_len"].tolist() == [2, 2, 0] and recs["first"].tolist() == [5, 0, 1]
    files, sup = file_records([FileRecord(0, 2, 1, [bytes([1]) * 32]), FileRecord(2, 1),
                               FileRecord(3, 0, 0, [])])
    assert files["has_supersedes"].tolist() == [1, 0, 1] and sup.shape == (1, 32)
    assert files["sup_count"].tolist() == [1, 0, 0]
    for bad in (PackRecord(b"short", 0, 0, 0), PackRecord(bytes(32), 0, 0, 0, None, 1 << 32),
                PackRecord(bytes(32), 0, -1, 0)):
        with pytest.raises(RusticError):
            pack_records([bad])
    with pytest.raises(RusticError):
        file_records([FileRecord(0, 0, 0, [b"short"])])


# ---- PrunePlan.index_updates (prune.rs:1230-1353) -----------------------------------

PRUNE_TIME = "2024-05-01T12:00:00+00:00"


def _table_plan(instant_delete):
    """One pack per PackToDo value but Undecided, each with and without a
    prior time where the decision allows it, decided by the real plan on the
    host engine; two packs no index file knows."""
    from rustic_core_amd.prune import PruneOptions
    from tests.prune_cases import OLD, YOUNG, bid, existing_of, one_file, pack, plan_of
    files = [
        one_file([pack("keep_t", [("a", 10)], time=OLD), pack("keep_n", [("b", 10)]),
                  pack("repack_t", [("c", 10), ("x1", 20)], time=OLD),
                  pack("repack_n", [("d", 10), ("x2", 20)], tpe=1),
                  pack("markdel_t", [("x3", 5)], time=OLD), pack("markdel_n", [("x4", 5)], tpe=1)],
                 [pack("keepmarked", [("x5", 9)], time=YOUNG), pack("correct", [("x6", 9)]),
                  pack("recover_t", [("e", 3)], time=OLD), pack("recover_n", [("f", 3)], tpe=1),
                  pack("delete", [("x7", 1)], time=OLD)]),
    ]
    pairs = [(bid("index:0"), files[0])]
    existing = existing_of(pairs)
    existing[bid("pack:unref2")] = 222
    existing[bid("pack:unref1")] = 111
    opts = PruneOptions(max_unused="0%", max_repack="unlimited", no_resize=True,
                        instant_delete=instant_delete)
    return plan_of(files, list("abcdef"), device=None, opts=opts, existing=existing), bid


@pytest.mark.parametrize("instant_delete", [False, True])
def test_index_updates_table(instant_delete):
    from rustic_core_amd.index_write import PackRecord
    from rustic_core_amd.prune import DATA, TREE, PackToDo as T
    from tests.prune_cases import OLD, YOUNG
    plan, bid = _table_plan(instant_delete)
    todo = {p.id: p.to_do for p in plan.packs}
    name = lambda n: bid("pack:" + n)
    assert [todo[name(n)] for n in ("keep_t", "keep_n", "repack_t", "repack_n", "markdel_t",
                                    "markdel_n", "keepmarked", "correct", "recover_t",
                                    "recover_n", "delete")] == \
        [T.Keep, T.Keep, T.Repack, T.Repack, T.MarkDelete, T.MarkDelete, T.KeepMarked,
         T.KeepMarkedAndCorrect, T.Recover, T.Recover, T.Delete]
    assert len(plan.index_files) == 1
    where = {p.id: (p.first, p.count) for p in plan.packs}
    unref = sorted([name("unref1"), name("unref2")])
    assert list(plan.existing_packs) == unref
    up = plan.index_updates(PRUNE_TIME, instant_delete)

    def rec(n, tpe, time):
        return PackRecord(name(n), tpe, where[name(n)][0], where[name(n)][1], time, None)
    # prune.rs:1246-1255: a removal record per unreferenced pack, in id order
    removal = [(PackRecord(i, DATA, 0, 0, PRUNE_TIME, plan.existing_packs[i]), True) for i in unref]
    assert sorted(plan.existing_packs.values()) == [111, 222]
    if not instant_delete:
        assert up.adds == removal + [
            (rec("keep_t", DATA, OLD), False),            # :1307-1311 into_index_pack
            (rec("keep_n", DATA, PRUNE_TIME), False),     #   time.or(prune_time)
            (rec("repack_t", DATA, PRUNE_TIME), True),    # :1317-1318 with_time, add_remove
            (rec("repack_n", TREE, PRUNE_TIME), True),
            (rec("markdel_t", DATA, PRUNE_TIME), True),   # :1331-1332
            (rec("markdel_n", TREE, PRUNE_TIME), True),
            (rec("keepmarked", DATA, YOUNG), True),       # :1341-1342 keeps the timestamp
            (rec("correct", DATA, PRUNE_TIME), True),     #   and heals a missing one
            (rec("recover_t", DATA, PRUNE_TIME), False),  # :1347-1348 with_time, add
            (rec("recover_n", TREE, PRUNE_TIME), False),
        ]
        assert up.delete_packs == {DATA: [name("delete")], TREE: []}  # :1350
        assert up.delete_unindexed == []
    else:
        assert up.adds == [
            (rec("keep_t", DATA, OLD), False),
            (rec("keep_n", DATA, PRUNE_TIME), False),
            (rec("recover_t", DATA, PRUNE_TIME), False),
            (rec("recover_n", TREE, PRUNE_TIME), False),
        ]
        assert up.delete_packs == {                        # :1282-1288 per type, in pack order
            DATA: [name(n) for n in ("repack_t", "markdel_t", "keepmarked", "correct", "delete")],
            TREE: [name(n) for n in ("repack_n", "markdel_n")]}
        assert up.delete_unindexed == unref                # :1233-1236
    assert all(r.size is None for r, _ in up.adds[len(removal) if not instant_delete else 0:])


def test_index_updates_undecided_raises():
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.prune import PackToDo
    plan, _ = _table_plan(False)
    plan.index_files[0].packs[3].to_do = PackToDo.Undecided
    with pytest.raises(RusticError) as e:
        plan.index_updates(PRUNE_TIME, False)
    assert e.value.kind == ErrorKind.Internal and "got no decision what to do with it!" in str(e.value)


# ---- DeviceIndexer's split rule -------------------------------------------------------

def _host_pack(seed, n_blobs, tpe=0, time=None):
    from rustic_core_amd.index import IndexPack
    p = IndexPack(bytes([seed % 256]) * 32, time=time)
    for j in range(n_blobs):
        p.add(bytes([seed % 256, j % 256]) * 16, tpe, j, j + 1, (j % 3) or None)
    return p


def _captured(monkeypatch):
    """write_json / save_index_files replaced: every batch as the IndexFiles
    its records and arrays describe."""
    from rustic_core_amd import index_write
    from rustic_core_amd.index import IndexBlob, IndexFile, IndexPack
    batches = []

    def fake_write(ids, offsets, lens, ulens, packs, files, device=0, guard=0):
        out = []
        for f in files:
            g = IndexFile(supersedes=f.supersedes)
            for k in range(f.pack_first, f.pack_first + f.pack_count):
                r = packs[k]
                p = IndexPack(r.id, time=r.time, size=r.size)
                for e in range(r.first, r.first + r.count):
                    p.blobs.append(IndexBlob(bytes(ids[e]), r.type, int(offsets[e]), int(lens[e]),
                                             int(ulens[e]) or None))
                g.add(p, delete=k >= f.pack_first + f.pack_count - f.n_delete)
            out.append(g)
        return out

    def fake_save(key, written, version=2, level=0, nonces=None, device=0, stage_times=None):
        batches.append(written)
        return [b"id%d" % i for i in range(len(written))], None, None, None
    monkeypatch.setattr(index_write, "write_json", fake_write)
    monkeypatch.setattr(index_write, "save_index_files", fake_save)
    return batches


@pytest.mark.parametrize("flush_files", [None, 1, 3])
def test_device_indexer_splits_as_indexer_does(monkeypatch, flush_files):
    from rustic_core_amd import index
    from rustic_core_amd.index_write import DeviceIndexer, PackRecord
    batches = _captured(monkeypatch)
    sizes = [0, 1, 999, 1, 1, 1000, 2500, 3, 0, 0, 400, 400, 199, 1, 0, 7, 1001, 5]
    packs = [_host_pack(i, n, i % 2, "t%d" % i if i % 3 else None) for i, n in enumerate(sizes)]
    deletes = [i % 4 == 1 for i in range(len(packs))]
    assert max(sizes) > 2 * 1000  # a pack that alone exceeds max_count
    monkeypatch.setattr(index, "MAX_COUNT", 1000)
    want = []
    host = index.Indexer(lambda f: want.append(f) or b"")
    for p, d in zip(packs, deletes):
        host.add(p, d)
    host.finalize()
    assert len(want) == 6 and sum(len(f.packs) + len(f.packs_to_delete) for f in want) == len(packs)
    # records into numpy entry arrays for the even packs, host packs for the odd ones
    ids, ints, recs = [], [], {}
    for i, p in enumerate(packs):
        if i % 2 == 0:
            recs[i] = PackRecord(p.id, i % 2, len(ids), len(p.blobs), p.time, p.size)
            ids += [b.id for b in p.blobs]
            ints += [(b.offset, b.length, b.uncompressed_length or 0) for b in p.blobs]
    a = np.array(ints, np.uint32)
    entries = (np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32), a[:, 0], a[:, 1], a[:, 2])
    calls = []
    ix = DeviceIndexer(lambda *args: calls.append(args[0]), max_count=1000, key=object(),
                       entries=entries, flush_files=flush_files)
    for i, (p, d) in enumerate(zip(packs, deletes)):
        ix.add(recs[i] if i in recs else p, d)
        assert not ix.has(p.blobs[0].id if p.blobs else bytes(32))
    ix.finalize()
    got = [f for b in batches for f in b]
    assert [f.to_json() for f in got] == [f.to_json() for f in want]
    assert len(batches) == {None: 1, 1: 6, 3: 2}[flush_files] == len(calls)
    assert ix.saved == [i for c in calls for i in c] and len(ix.saved) == 6


def test_device_indexer_empty_finalize_and_has(monkeypatch):
    from rustic_core_amd.errors import RusticError
    from rustic_core_amd.index_write import DeviceIndexer, PackRecord
    batches = _captured(monkeypatch)
    calls = []
    ix = DeviceIndexer(lambda *a: calls.append(a), max_count=1000, key=object())
    ix.finalize()
    ix.finalize()
    assert batches == [] and calls == [] and ix.saved == []
    # has() answers for host packs when a set is given, as Indexer does
    ix = DeviceIndexer(lambda *a: calls.append(a), max_count=10, key=object(), indexed=set())
    p = _host_pack(3, 4)
    ix.add(p)
    assert ix.has(p.blobs[2].id) and not ix.has(bytes(32))
    ix.add_remove(_host_pack(4, 2))
    ix.finalize()
    assert len(batches) == 1 and len(batches[0]) == 1
    assert [len(x.blobs) for x in batches[0][0].packs] == [4]
    assert [len(x.blobs) for x in batches[0][0].packs_to_delete] == [2]
    # a record without entry arrays, a pack of two types, no key
    with pytest.raises(RusticError):
        DeviceIndexer(None, key=object()).add(PackRecord(bytes(32), 0, 0, 1))
    mixed = _host_pack(5, 2)
    mixed.blobs[1].type = 1
    with pytest.raises(RusticError):
        DeviceIndexer(None, key=object()).add(mixed)
    ix = DeviceIndexer(None, max_count=1)
    ix.add(_host_pack(6, 1))
    with pytest.raises(RusticError):
        ix.finalize()
