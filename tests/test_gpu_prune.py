"""GPU: prune's plan with the per-blob part on the device (rcdc_prune in
include/rcdc.h, rustic_core_amd.prune.DevicePrune) against the same plan
with that part on the host (``device=None``, HostPrune): every output is
compared."""
import ctypes
import hashlib

import numpy as np
import pytest

from rustic_core_amd import _lib
from rustic_core_amd.errors import ErrorKind, RusticError
from rustic_core_amd.prune import (DevicePrune, HostPrune, PACK, RANGE, PackToDo, PruneOptions)

from tests.prune_cases import (CASES, OLD, YOUNG, bid, case_files, chain, ids_array, one_file, pack,
                               plan_of, plan_summary, random_repo)

pytestmark = pytest.mark.gpu

INVALID = 2  # RCDC_ERR_INVALID_INPUT


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def both(files, used, **kw):
    host = plan_of(files, used, device=None, **kw)
    dev = plan_of(files, used, device=0, **kw)
    hs, ds = plan_summary(host), plan_summary(dev)
    for k in hs:
        assert hs[k] == ds[k], k
    return host, dev


def raw_both(ids, lens, ulens, ranges, used, kinds=None, rank=None, tensors=None):
    """DevicePrune against HostPrune over arrays; returns the host's outputs
    and the device's result record."""
    torch, dev = _torch()
    h = HostPrune(used)
    h.set_entries(ids, lens, ulens, ranges)
    hc, hu, hp, hr = h.mark()
    d = DevicePrune(torch.from_numpy(np.ascontiguousarray(used)).to(dev))
    if tensors is None:
        tensors = (torch.from_numpy(np.ascontiguousarray(ids)).to(dev),
                   torch.from_numpy(np.asarray(lens, np.uint32).view(np.int32).copy()).to(dev),
                   torch.from_numpy(np.asarray(ulens, np.uint32).view(np.int32).copy()).to(dev))
    d.set_entries(*tensors, ranges)
    dc, du, dp, dr = d.mark()
    assert dc.cpu().numpy().tolist() == hc.tolist()
    assert du.cpu().numpy().tolist() == hu.tolist()
    for f in ("used_blobs", "unused_blobs", "used_size", "unused_size", "compressed"):
        assert dp[f].tolist() == hp[f].tolist(), f
    assert (dr.missing, dr.first_missing) == (hr.missing, hr.first_missing)
    assert dr.rounds <= len(ranges) + 1
    if kinds is None:
        rng = np.random.default_rng(len(ranges))
        kinds = rng.integers(0, 3, len(ranges)).astype(np.uint8)
        rank = rng.permutation(len(ranges)).astype(np.uint32)
    assert d.keep(kinds, rank).cpu().numpy().tolist() == h.keep(kinds, rank).tolist()
    d.close()
    return hc, hu, hp, dr


@pytest.mark.parametrize("name", sorted(CASES))
def test_marking_cases(gpu_ctx, name):
    files, used, infos, flags = case_files(name)
    _, dev = both(files, used)
    assert [p.info.sums() for p in dev.packs] == infos and dev.used.tolist() == flags


@pytest.mark.parametrize("time,want", [(OLD, PackToDo.Delete), (YOUNG, PackToDo.KeepMarked),
                                       (None, PackToDo.KeepMarkedAndCorrect)])
def test_case_h(gpu_ctx, time, want):
    f = one_file([pack("P", [("a", 10)])], [pack("M", [("a", 10)], time=time)])
    _, dev = both([f], ["a"])
    assert dev.counts.tolist() == [2]
    assert [p.to_do for p in dev.packs] == [PackToDo.Keep, want]


@pytest.mark.parametrize("seed", range(5))
def test_random_repositories(gpu_ctx, seed):
    files, used = random_repo(seed)
    opts = PruneOptions(max_unused="0%", max_repack="unlimited") if seed % 2 else PruneOptions()
    host, dev = both(files, used, opts=opts)
    assert dev.rounds >= 1 and len(dev.packs) == 201
    assert len({p.to_do for p in dev.packs}) >= 4  # the decisions are not all alike


def test_chain(gpu_ctx):
    files, used = chain(4096)
    host, dev = both(files, used)
    # every second pack is needed; the last one holds the one id nobody else has
    assert [p.info.used_blobs for p in dev.packs[:4]] == [2, 0, 2, 0]
    assert [p.info.used_blobs for p in dev.packs[-2:]] == [2, 1]
    assert 1 <= dev.rounds <= 4096 + 1


@pytest.mark.parametrize("where", [0, 100, 300])
def test_saturation(gpu_ctx, where):
    """One id in 300 one-blob packs, and once more among 64 other ids in one
    wave's worth of entries."""
    ones = [pack("one%d" % i, [("a", 1 + i % 7)]) for i in range(300)]
    others = [("o%d" % i, 3) for i in range(64)]
    wave = pack("wave", others[:40] + [("a", 9)] + others[40:])
    packs = ones[:where] + [wave] + ones[where:]
    host, dev = both([one_file(packs)], ["a"] + [n for n, _ in others[::2]])
    assert dev.counts.tolist()[0] == 255


def _random_arrays(rng, n, pool):
    ids = ids_array(["g%d" % i for i in rng.integers(0, pool, n)])
    lens = rng.integers(1, 1 << 20, n).astype(np.uint32)
    ulens = np.where(rng.integers(0, 8, n) == 0, 0, lens * 2).astype(np.uint32)
    return ids, lens, ulens


def test_ranges_out_of_order_with_gaps(gpu_ctx):
    rng = np.random.default_rng(7)
    n = 3000
    ids, lens, ulens = _random_arrays(rng, n, 400)
    # ranges cut from the array with gaps between them, then shuffled
    ranges, at = [], 5
    while at < n - 70:
        c = int(rng.integers(0, 60))
        ranges.append((at, c))
        at += c + int(rng.integers(0, 9))
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    used = ids_array(["g%d" % i for i in range(0, 400, 2)])
    hc, hu, hp, _ = raw_both(ids, lens, ulens, ranges, used)
    covered = np.zeros(n, bool)
    for f, c in ranges:
        covered[f:f + c] = True
    assert not covered.all() and not hu[~covered].any()
    # the gaps count for nothing: the same ids with the gaps' ids changed
    ids2 = ids.copy()
    ids2[~covered] = ids_array(["g1"])[0]
    hc2, hu2, _, _ = raw_both(ids2, lens, ulens, ranges, used)
    assert hc2.tolist() == hc.tolist() and hu2.tolist() == hu.tolist()


def test_strided_arrays(gpu_ctx):
    """ids and a d_locs-shaped (n, 4) tensor: columns 2 and 3 are the
    lengths; the results are those of the contiguous run."""
    torch, dev = _torch()
    rng = np.random.default_rng(11)
    n = 2000
    ids, lens, ulens = _random_arrays(rng, n, 300)
    ranges = [(i, 50) for i in range(0, n, 50)]
    used = ids_array(["g%d" % i for i in range(0, 300, 3)])
    locs = np.zeros((n, 4), np.uint32)
    locs[:, 0], locs[:, 1], locs[:, 2], locs[:, 3] = 7, rng.integers(0, 1 << 30, n), lens, ulens
    d_locs = torch.from_numpy(locs.view(np.int32)).to(dev)
    wide = torch.zeros((n, 48), dtype=torch.uint8, device=dev)   # ids with a stride of 48
    wide[:, 8:40] = torch.from_numpy(ids).to(dev)
    a = raw_both(ids, lens, ulens, ranges, used)
    b = raw_both(ids, lens, ulens, ranges, used,
                 tensors=(torch.from_numpy(ids).to(dev), d_locs[:, 2], d_locs[:, 3]))
    c = raw_both(ids, lens, ulens, ranges, used, tensors=(wide[:, 8:40], d_locs[:, 2], d_locs[:, 3]))
    for x in (b, c):
        assert x[0].tolist() == a[0].tolist() and x[1].tolist() == a[1].tolist()


def test_crafted_ids(gpu_ctx):
    """Used ids that share a home slot of the table, and ids with equal
    tags (test_gpu_dindex.py::test_colliding_ids), at 300 ids."""
    sha = lambda *a: hashlib.sha256(repr(a).encode()).digest()
    same_home = [b"\x37\x13\x00\x00\x00\x00\x00\x00" + sha("home", k)[8:] for k in range(300)]
    t = sha("tag")
    same_tag = [sha("t1", k)[:8] + t[8:12] + sha("t2", k)[12:] for k in range(300)]
    near = [i[:31] + bytes([i[31] ^ 1]) for i in same_home[:50]]
    pool = same_home + same_tag + near
    rng = np.random.default_rng(3)
    n = 2400
    ids = np.frombuffer(b"".join(pool[i] for i in rng.integers(0, len(pool), n)),
                        np.uint8).reshape(n, 32).copy()
    lens = rng.integers(1, 1000, n).astype(np.uint32)
    used = np.frombuffer(b"".join(same_home + same_tag), np.uint8).reshape(600, 32).copy()
    hc, hu, _, _ = raw_both(ids, lens, lens, [(i, 30) for i in range(0, n, 30)], used)
    assert hu.sum() > 300


def test_edge_shapes(gpu_ctx):
    rng = np.random.default_rng(5)
    ids, lens, ulens = _random_arrays(rng, 40, 10)
    used = ids_array(["g%d" % i for i in range(10)])
    none = np.zeros((0, 32), np.uint8)
    z = np.zeros(0, np.uint32)
    raw_both(ids, lens, ulens, [(0, 20), (20, 20)], none)           # m = 0
    raw_both(none, z, z, [], used)                                   # n = 0, zero packs
    raw_both(none, z, z, [(0, 0), (0, 0)], used)                     # n = 0, empty packs
    raw_both(ids, lens, ulens, [], used)                             # zero packs
    _, _, hp, _ = raw_both(ids, lens, ulens, [(0, 10), (10, 0), (10, 30)], used)  # an empty pack
    assert hp["compressed"][1] == 1 and hp["used_blobs"][1] == 0


def test_invalid_input(gpu_ctx):
    """Every rejected input returns the invalid-input status and leaves the
    outputs as they were."""
    torch, dev = _torch()
    L = _lib.lib()
    rng = np.random.default_rng(9)
    n = 100
    ids, lens, ulens = _random_arrays(rng, n, 30)
    used = torch.from_numpy(ids_array(["g%d" % i for i in range(30)])).to(dev)
    d = DevicePrune(used)
    t_ids = torch.from_numpy(ids).to(dev)
    t_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    t_ulen = torch.from_numpy(ulens.view(np.int32)).to(dev)
    counts = torch.full((30,), 0xA5, dtype=torch.uint8, device=dev)
    flags = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    packs = np.full(4, 0xA5, np.uint8).repeat(PACK.itemsize).view(PACK)
    res = _lib.PruneResult()

    def ranges(*r):
        a = np.zeros(len(r), RANGE)
        for i, (f, c) in enumerate(r):
            a[i] = (f, c, 0)
        return a

    def set_entries(r, n=n, ids=t_ids.data_ptr(), ln=t_len.data_ptr(), ul=t_ulen.data_ptr(),
                    s_len=4, handle=d.handle):
        return L.rcdc_prune_set_entries(handle, ids, 32, ln, s_len, ul, 4, n,
                                        r.ctypes.data if len(r) else None, len(r), None)

    def untouched():
        torch.cuda.synchronize()
        assert (counts.cpu().numpy() == 0xA5).all() and (flags.cpu().numpy() == 0xA5).all()
        assert (packs.view(np.uint8) == 0xA5).all()

    ok = ranges((0, 50), (50, 50))
    assert set_entries(ranges((0, 50), (60, 41))) == INVALID          # past the entries
    assert set_entries(ranges((0, 50), (49, 10))) == INVALID          # overlap
    assert set_entries(ranges((0, 50), (10, 5))) == INVALID           # one inside another
    assert set_entries(ranges((0, 65536))) == INVALID                 # a pack too large
    assert set_entries(ok, n=(1 << 32) - 1) == INVALID
    assert set_entries(ok, ids=None) == INVALID
    assert set_entries(ok, ln=None) == INVALID
    assert set_entries(ok, ul=None) == INVALID
    assert set_entries(ok, ln=t_len.data_ptr() + 1) == INVALID        # unaligned lengths
    assert set_entries(ok, s_len=6) == INVALID
    assert set_entries(ok, handle=None) == INVALID
    assert L.rcdc_prune_set_entries(d.handle, t_ids.data_ptr(), 32, t_len.data_ptr(), 4,
                                    t_ulen.data_ptr(), 4, n, None, 2, None) == INVALID
    # nothing was set: mark and keep refuse too
    mark = lambda c=counts.data_ptr(), f=flags.data_ptr(), p=packs.ctypes.data, r=ctypes.byref(res), \
        h=d.handle: L.rcdc_prune_mark(h, c, f, p, r, None)
    assert mark() == INVALID
    untouched()
    assert set_entries(ok) == 0
    assert mark(c=None) == INVALID and mark(f=None) == INVALID and mark(p=None) == INVALID
    assert mark(r=None) == INVALID and mark(h=None) == INVALID
    kinds, rank = np.array([2, 1], np.uint8), np.array([1, 0], np.uint32)
    keep = lambda k=kinds, r=rank, o=flags.data_ptr(): L.rcdc_prune_keep(
        d.handle, None if k is None else k.ctypes.data, None if r is None else r.ctypes.data, o, None)
    assert keep(k=np.array([3, 0], np.uint8)) == INVALID
    assert keep(r=np.array([1, 1], np.uint32)) == INVALID
    assert keep(r=np.array([0, 2], np.uint32)) == INVALID
    assert keep(k=None) == INVALID and keep(r=None) == INVALID and keep(o=None) == INVALID
    untouched()
    assert "rcdc_prune" in _lib.last_error()
    # used ids that repeat, too many of them
    h = ctypes.c_void_p()
    from rustic_core_amd.crypto import _ctx
    twice = torch.cat([used, used[:1]])
    assert L.rcdc_prune_create(_ctx(0).handle, twice.data_ptr(), 31, None, ctypes.byref(h)) == INVALID
    assert L.rcdc_prune_create(_ctx(0).handle, used.data_ptr(), (1 << 32) - 1, None,
                               ctypes.byref(h)) == INVALID
    assert L.rcdc_prune_create(_ctx(0).handle, None, 3, None, ctypes.byref(h)) == INVALID
    assert L.rcdc_prune_create(None, used.data_ptr(), 30, None, ctypes.byref(h)) == INVALID
    # and the handle still works
    assert mark() == 0 and keep() == 0
    torch.cuda.synchronize()
    assert set(flags.cpu().numpy().tolist()) <= {0, 1}
    d.close()
    with pytest.raises(RusticError) as e:
        plan_of([one_file([pack("big", [("b%d" % i, 1) for i in range(65536)])])], ["b0"], device=0)
    assert e.value.kind == ErrorKind.InvalidInput


def test_missing_blob(gpu_ctx):
    with pytest.raises(RusticError) as e:
        plan_of([one_file([pack("P", [("a", 10)])])], ["a", "nowhere", "nowhere2"], device=0)
    assert e.value.kind == ErrorKind.Internal and bid("nowhere").hex() in e.value.message


def test_end_to_end_repack(gpu_ctx):
    """Three packs of the repack tests' source; half of one pack's blobs are
    unused; the plan's repack_plans() through BlobCopier with the plan's
    sizer: the new packs hold the used blobs of that pack, each once."""
    from rustic_core_amd.chunker import ConfigFile
    from rustic_core_amd.index import IndexFile
    from tests.test_gpu_repack import _SOURCE, KEY, Source, _check_packs, _copier
    if not _SOURCE:
        _SOURCE.append(Source())
    src = _SOURCE[0]
    names = ["zstd", "tree", "mixed"]
    mixed = src.index["mixed"].blobs
    used = [b.id for n in names[:2] for b in src.index[n].blobs] + [b.id for b in mixed[::2]]
    files = [(bid("index:0"), IndexFile(packs=[src.index[n] for n in names]))]
    existing = {src.index[n].id: len(src.packs[src.index[n].id]) for n in names}
    u = np.frombuffer(b"".join(used), np.uint8).reshape(len(used), 32).copy()
    plans = {}
    for device in (None, 0):
        from rustic_core_amd.prune import PrunePlan
        from tests.prune_cases import NOW
        plans[device] = PrunePlan.from_index_files(
            files, u, existing, PruneOptions(max_unused="0%", max_repack="unlimited",
                                             no_resize=True), ConfigFile(version=2), NOW,
            device=device)
    plan = plans[0]
    assert plan_summary(plan) == plan_summary(plans[None])
    assert plan.repack_packs() == [src.index["mixed"].id]
    c = _copier(level=0)
    c.sizer = plan.pack_sizers()[0]
    new = []
    for p, reads in plan.repack_plans():
        new += c.copy(reads, src.reader())
    new += c.finalize()
    ids = _check_packs(KEY, new)
    assert sorted(ids) == sorted(b.id for b in mixed[::2])


def test_from_entries_over_parsed_json(gpu_ctx):
    """The device parser's arrays go into the plan as they are (ids, and the
    columns of locs as strided views); only per-pack records are host
    objects.  Pack times come from the host (the parser does not give them)."""
    import torch
    from rustic_core_amd import dindex
    from rustic_core_amd.index import IndexFile
    from rustic_core_amd.prune import PrunePack, PrunePlan
    from tests.prune_cases import CONFIG, NOW, existing_of
    from tests.test_gpu_index_parse import _arena
    files, used = random_repo(3)
    files = [(bid("index:%d" % i), IndexFile(packs=f.packs + f.packs_to_delete))
             for i, f in enumerate(files)]
    opts = PruneOptions(max_unused="0%", max_repack="unlimited")
    want = plan_summary(PrunePlan.from_index_files(files, ids_array(used), existing_of(files), opts,
                                                   CONFIG, NOW, device=None))
    d_json, offs, lens = _arena([f.to_json() for _, f in files], align=16)
    res = dindex.parse_json(d_json, offs, lens)
    assert res.files["status"].tolist() == [dindex.PARSED] * len(files)
    e = res.entries
    ids = torch.cat([res.ids[t][:e[t]] for t in (0, 1)])
    locs = torch.cat([res.locs[t][:e[t]] for t in (0, 1)])
    per_type = [int((res.packs["type"] == t).sum()) for t in (0, 1)]
    counts = [torch.bincount(res.locs[t][:e[t], 0], minlength=per_type[t]).cpu().numpy()
              for t in (0, 1)]
    firsts = [np.concatenate([[0], np.cumsum(c)[:-1]]) + base if len(c) else c
              for c, base in zip(counts, (0, e[0]))]
    times = {p.id: p.time for _, f in files for p in f.packs}
    file_of = np.repeat(np.arange(len(files)), res.files["packs"].sum(axis=1).astype(np.int64))
    recs = [PrunePack(p["id"].tobytes(), int(p["type"]), int(p["size"]), times[p["id"].tobytes()],
                      False, int(file_of[k]), int(firsts[int(p["type"])][int(p["number"])]),
                      int(counts[int(p["type"])][int(p["number"])]))
            for k, p in enumerate(res.packs)]
    plan = PrunePlan.from_entries(ids, locs[:, 2], locs[:, 3], locs[:, 1], recs,
                                  [i for i, _ in files], torch.from_numpy(ids_array(used)).to("cuda:0"),
                                  existing_of(files), opts, CONFIG, NOW, device=0)
    got = plan_summary(plan)
    for k in want:
        if k not in ("used", "keep"):  # per entry, and the entries are ordered by type here
            assert got[k] == want[k], k
    assert sum(got["used"]) == sum(want["used"]) and sum(got["keep"]) == sum(want["keep"])
