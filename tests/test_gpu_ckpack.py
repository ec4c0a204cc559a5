"""GPU: rcdc_check_packs (include/rcdc.h) against the model of its rule
(tests/ckpack_model.py), with 0xA5 guard bytes behind every device output."""
import types as pytypes

import numpy as np
import pytest

from tests import ckpack_model as cm

pytestmark = pytest.mark.gpu
GUARD = 64


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _cat(packs):
    ids = np.concatenate([p[0] for p in packs]) if packs else np.zeros((0, 32), np.uint8)
    locs = np.concatenate([p[1] for p in packs]) if packs else np.zeros((0, 4), np.uint32)
    tps = np.concatenate([p[2] for p in packs]) if packs else np.zeros(0, np.uint8)
    ranges, at = [], 0
    for p in packs:
        ranges.append((at, len(p[0])))
        at += len(p[0])
    return ids, locs, tps, ranges


def _run(ids, locs, tps, ranges, hdr=None, cap=None, use_types=True, want_order=True):
    """The kernel and the model over the same arrays, compared in full.
    ``want_order`` off: no order array, and the emit pass lists only the packs
    with findings or a header."""
    from rustic_core_amd.check import CK_FINDING, run_check_packs, sort_max
    d_ids, d_locs = _dev(ids), _dev(locs.view(np.int32))
    d_types = _dev(tps) if use_types else None
    dh = None
    if hdr is not None:
        parsed = pytypes.SimpleNamespace(ids=[_dev(a) for a in hdr[0]],
                                         locs=[_dev(a.view(np.int32)) for a in hdr[1]],
                                         entries=[len(a) for a in hdr[0]])
        recs = np.array([(t, c, f) for t, c, f in hdr[2]],
                        np.dtype([("type", "<u4"), ("count", "<u4"), ("first", "<u8")]))
        dh = (parsed, recs)
    res = run_check_packs(d_ids, d_locs[:, 1], d_locs[:, 2], d_locs[:, 3], d_types, ranges, hdr=dh,
                          cap_findings=cap, want_order=want_order, guard=GUARD)
    packs, findings, order = cm.model(ids, locs, tps if use_types else None, ranges, sort_max(), hdr)
    for p, (got, want) in enumerate(zip(res.packs, packs)):
        for k, v in want.items():
            assert int(got[k]) == v, (p, k, int(got[k]), v)
    assert res.total == len(findings)
    assert res.packs_host == sum(p["status"] == cm.HOST for p in packs)
    assert res.packs_sorted_on_device == sum(p["status"] == cm.OK and not p["sorted"] for p in packs)
    written = min(len(findings), int(res.findings.shape[0]))
    got = res.findings_host()
    assert [tuple(int(x) for x in f) for f in got] == findings[:written]
    # behind the written records nothing was touched, nor behind any output
    raw_f = res.raw[-1].cpu().numpy()
    assert (raw_f[written * CK_FINDING.itemsize:] == 0xA5).all()
    if not want_order:
        assert res.order is None and len(res.raw) == 1
        return res, packs, findings
    raw_o = res.raw[0].cpu().numpy()
    assert (raw_o[len(ids) * 4:] == 0xA5).all()
    rows = raw_o[:len(ids) * 4].view(np.uint32)
    want_rows = np.full(len(ids), 0xA5A5A5A5, np.uint32)  # rows outside every OK pack: untouched
    if order:
        want_rows[np.fromiter(order.keys(), np.int64)] = np.fromiter(order.values(), np.int64)
    assert np.array_equal(rows, want_rows)
    return res, packs, findings


def test_sizes_orders_and_findings():
    """Packs of 0 to 257 entries, in order and shuffled, with a gap, an
    overlap, equal locations, a wrapping offset and wrong type bytes, at
    scrambled places of the arrays; then the same with one record of room too
    few."""
    rng = np.random.default_rng(3)
    packs = []
    for i, n in enumerate([0, 1, 2, 63, 64, 65, 255, 256, 257]):
        packs.append(cm.random_pack(rng, n, shuffle=False, gap=i % 3 == 1, types=i & 1))
        packs.append(cm.random_pack(rng, n, shuffle=True, gap=i % 3 == 2, types=~i & 1))
    ids, locs, tps, ranges = _cat(packs)
    # an overlap of two blobs, equal locations, a length that wraps 2^32
    f, c = ranges[7]   # 63 shuffled
    locs[f + 5, 1] -= 9
    locs[f + 9] = locs[f + 30]
    locs[f + 31] = locs[f + 30]
    f, c = ranges[10]  # 65 in order
    locs[f + 20, 2] = 0xFFFFFF00
    # one wrong type byte in the first, the middle and the last entry
    for r in (12, 13, 14):
        f, c = ranges[r]
        tps[f + {12: 0, 13: c // 2, 14: c - 1}[r]] ^= 1
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    res, model_packs, findings = _run(ids, locs, tps, ranges)
    assert len(findings) > 200 and res.packs_sorted_on_device >= 7
    _run(ids, locs, tps, ranges, cap=len(findings) - 1)
    _run(ids, locs, tps, ranges, cap=0)
    _run(ids, locs, None, ranges, use_types=False)


def test_large_packs_and_the_host_status():
    """A pack of 70 000 entries in order at any count; a shuffled pack of
    exactly SORT_MAX entries sorted on the device; one of SORT_MAX + 1 is the
    host's, and the packs on either side of it stay right."""
    from rustic_core_amd.check import sort_max
    rng = np.random.default_rng(4)
    m = sort_max()
    assert m >= 4096
    packs = [cm.random_pack(rng, 70_000, gap=True), cm.random_pack(rng, 300, shuffle=True),
             cm.random_pack(rng, m + 1, shuffle=True), cm.random_pack(rng, m, shuffle=True, gap=True),
             cm.random_pack(rng, 70_001, shuffle=True), cm.random_pack(rng, 5, gap=True)]
    res, model_packs, findings = _run(*_cat(packs))
    assert [p["status"] for p in model_packs] == [0, 0, 1, 0, 1, 0]
    assert [p["sorted"] for p in model_packs] == [1, 0, 0, 0, 0, 1]
    assert model_packs[0]["offset_findings"] == 35_000 and model_packs[3]["offset_findings"] == m // 2


def _with_headers(rng, counts):
    packs = [cm.random_pack(rng, n, shuffle=bool(i & 1), types=i % 2) for i, n in enumerate(counts)]
    ids, locs, tps, ranges = _cat(packs)
    return ids, locs, tps, ranges, _headers_of(ids, locs, tps, ranges)


def _headers_of(ids, locs, tps, ranges):
    """The headers of the packs as their packer wrote them: every pack's
    entries in pack order, under the type of its first entry."""
    h_ids, h_locs, recs = [[], []], [[], []], []
    for (f, c) in ranges:
        t = int(tps[f]) if c else 0
        rows = cm.pack_order(locs, f, c)
        recs.append((t, c, sum(len(x) for x in h_ids[t])))
        h_ids[t].append(ids[rows])
        h_locs[t].append(locs[rows])
    cat = lambda parts, w, dt: (np.concatenate(parts) if parts else np.zeros((0, w), dt)).copy()
    return ([cat(p, 32, np.uint8) for p in h_ids], [cat(p, 4, np.uint32) for p in h_locs], recs)


def test_header_compare():
    """EQUAL for every pack against its own sorted entries, then one pack
    each that differs in the last byte of the last id, in one uncompressed
    length, in the count by one (either way) and in the type; a pack without
    a header is NOT_COMPARED."""
    rng = np.random.default_rng(5)
    counts = [0, 1, 64, 200, 257, 300, 31, 90, 91]
    ids, locs, tps, ranges, hdr = _with_headers(rng, counts)
    res, packs, _ = _run(ids, locs, tps, ranges, hdr)
    assert all(p["header_verdict"] == cm.EQUAL for p in packs)
    h_ids, h_locs, recs = hdr
    t, c, f = recs[2]
    h_ids[t][f + c - 1, 31] ^= 1                    # the last byte of the last id
    t, c, f = recs[3]
    row = f + 100
    h_locs[t][row, 3] = 0 if h_locs[t][row, 3] else 77  # none against a length
    t, c, f = recs[4]
    recs[4] = (t, c - 1, f)                          # the header is a prefix
    t, c, f = recs[5]
    recs[5] = (t, c + 1, f)                          # the index is a prefix
    t, c, f = recs[6]
    recs[6] = (cm.NO_HEADER, 0, 0)
    t, c, f = recs[7]
    tps[ranges[7][0] + 40] ^= 1                      # one entry's type is not the header's
    # pack 8's header under the other type: every position differs
    t, c, f = recs[8]
    recs[8] = (t ^ 1, min(c, len(h_ids[t ^ 1])), 0)
    res, packs, _ = _run(ids, locs, tps, ranges, hdr)
    assert [p["header_verdict"] for p in packs] == [1, 1, 2, 2, 2, 2, 0, 2, 2]
    assert packs[2]["header_diff"] == 63 and packs[3]["header_diff"] == 100
    assert packs[4]["header_diff"] == 256 and packs[5]["header_diff"] == 300
    assert packs[8]["header_diff"] == 0
    # 0 and none are the same: an uncompressed length of 0 on both sides is EQUAL
    locs[ranges[1][0], 3] = 0
    hdr[1][recs[1][0]][recs[1][2], 3] = 0
    res, packs, _ = _run(ids, locs, tps, ranges, hdr)
    assert packs[1]["header_verdict"] == cm.EQUAL
    # without type bytes a pack has its header's type
    _run(ids, locs, None, ranges, hdr, use_types=False)


def test_more_packs_than_a_round(gpu_ctx):
    """4 300 packs of 0 to 6 entries: the sort list and the numbering take
    more than one round of 1024 packs (``carry``, ``listed``), the sort's grid
    of 1024 and the emit's of 4096 workgroups walk their lists with a stride.
    Packs with one wrong type byte and one offset gap stand on both sides of
    every round's edge, and around a pack that is the host's."""
    from rustic_core_amd.check import sort_max
    rng = np.random.default_rng(11)
    n_packs, host_at = 4300, 3000
    edges = (0, 1023, 1024, 1025, 2047, 2048, 4095, 4096, n_packs - 1)
    marked = edges + (host_at - 1, host_at + 1)
    differ = (4097, 4150, n_packs - 2)
    assert n_packs > 4 * 1024 + 1 and host_at > 2048 and min(differ) > 4096
    assert not set(marked) & set(differ)
    packs = []
    for pos in range(n_packs):
        if pos == host_at:
            packs.append(cm.random_pack(rng, sort_max() + 1, shuffle=True))
        elif pos in marked:
            n = int(rng.integers(4, 7))
            ids, locs, tps = cm.random_pack(rng, n, shuffle=bool(pos & 1), gap=True, types=pos % 2)
            tps[n - 1] ^= 1  # not the first entry, whose type is the pack's
            packs.append((ids, locs, tps))
        elif pos in differ:
            packs.append(cm.random_pack(rng, 3, shuffle=bool(pos & 1), types=pos % 2))
        else:
            n = int(rng.integers(0, 7))
            packs.append(cm.random_pack(rng, n, shuffle=bool(rng.integers(0, 2)), types=pos % 2))
    # the packs' entries lie in the arrays in another order than the ranges name them
    perm = rng.permutation(n_packs)
    ids, locs, tps, stored = _cat([packs[i] for i in perm])
    ranges = [None] * n_packs
    for j, pos in enumerate(perm):
        ranges[pos] = stored[j]
    assert [c for _, c in ranges] == [len(p[0]) for p in packs]

    res, model_packs, findings = _run(ids, locs, tps, ranges)
    shuffled = sum(p["status"] == cm.OK and not p["sorted"] for p in model_packs)
    assert shuffled > 1024 and res.packs_sorted_on_device == shuffled       # sort list, sort stride
    assert sum(p["status"] == cm.OK for p in model_packs) > 4096            # emit list, emit stride
    assert model_packs[host_at]["status"] == cm.HOST and res.packs_host == 1
    with_findings = [i for i, p in enumerate(model_packs) if p["type_findings"] + p["offset_findings"]]
    assert with_findings == sorted(marked)
    for i in marked:  # every entry behind the gap is off its expected offset
        n = ranges[i][1]
        assert (model_packs[i]["type_findings"], model_packs[i]["offset_findings"]) == (1, n - n // 2)
    assert len(findings) == sum(1 + ranges[i][1] - ranges[i][1] // 2 for i in marked)
    _run(ids, locs, tps, ranges, cap=len(findings) - 1)
    # without the order and without headers the emit list is the packs with findings alone:
    # a compaction over five rounds of the numbering
    assert len({i // 1024 for i in with_findings}) == 5
    _run(ids, locs, tps, ranges, want_order=False)
    _run(ids, locs, tps, ranges, want_order=False, cap=len(findings) - 1)

    hdr = _headers_of(ids, locs, tps, ranges)
    for i in differ:
        t, c, f = hdr[2][i]
        hdr[0][t][f + c - 1, 31] ^= 1  # the last byte of the last id
    res, model_packs, _ = _run(ids, locs, tps, ranges, hdr)
    for i, p in enumerate(model_packs):
        if i == host_at:
            want = (cm.NOT_COMPARED, 0)
        elif i in differ:
            want = (cm.DIFFERS, 2)
        elif i in marked:  # the entry of the wrong type byte is not the header's
            want = (cm.DIFFERS, p["header_diff"])
            assert int(tps[cm.pack_order(locs, *ranges[i])[p["header_diff"]]]) != p["type"]
        else:
            want = (cm.EQUAL, 0)
        assert (p["header_verdict"], p["header_diff"]) == want, i
    _run(ids, locs, tps, ranges, hdr, want_order=False)


def test_strided_columns_and_unaligned_ids():
    """Columns that are no rcdc_dindex_loc records, and id rows off a 16-byte
    boundary, give the same results (the plain loads)."""
    import torch
    from rustic_core_amd.check import run_check_packs
    from rustic_core_amd.check import CK_HDR
    rng = np.random.default_rng(6)
    ids, locs, tps, ranges, hdr = _with_headers(rng, [70, 300, 9])
    locs[ranges[1][0] + 50:ranges[1][0] + 300, 1] += 7  # a gap, in the index only
    hdr[0][1][299, 31] ^= 1                              # pack 1's header: its last id
    want, findings, _ = cm.model(ids, locs, tps, ranges, 4096, hdr)
    flat = torch.zeros(len(ids) * 32 + 8, dtype=torch.uint8, device="cuda:0")
    flat[8:] = _dev(ids).reshape(-1)
    d_ids = flat[8:].view(-1, 32)
    assert d_ids.data_ptr() % 16 == 8
    cols = [_dev(locs[:, c].copy().view(np.int32)) for c in (1, 2, 3)]
    parsed = pytypes.SimpleNamespace(ids=[_dev(a) for a in hdr[0]],
                                     locs=[_dev(a.view(np.int32)) for a in hdr[1]],
                                     entries=[len(a) for a in hdr[0]])
    res = run_check_packs(d_ids, cols[0], cols[1], cols[2], _dev(tps), ranges,
                          hdr=(parsed, np.array(hdr[2], CK_HDR)))
    assert [tuple(int(x) for x in f) for f in res.findings_host()] == findings and findings
    for k in ("end_offset", "header_verdict", "header_diff", "header_len"):
        assert [int(p[k]) for p in res.packs] == [p[k] for p in want], k
    assert [p["header_verdict"] for p in want] == [cm.EQUAL, cm.DIFFERS, cm.EQUAL]


def test_invalid_inputs():
    """Every invalid input is refused before anything is launched."""
    import ctypes
    import torch
    from rustic_core_amd import _lib
    from rustic_core_amd.check import CK_HDR, CK_PACK, CK_RANGE
    from rustic_core_amd.crypto import _ctx
    L, h = _lib.lib(), _ctx(0).handle
    n = 8
    ids = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    locs = torch.zeros((n, 4), dtype=torch.int32, device="cuda:0")
    res = _lib.CkpackResult()

    def call(ctx=h, d_ids=ids.data_ptr(), off=locs.data_ptr() + 4, ln=locs.data_ptr() + 8,
             ul=locs.data_ptr() + 12, strides=(32, 16, 16, 16), count=n, ranges=((0, 4), (4, 4)),
             hdr=None, result=res, packs=True, findings=(None, 0)):
        rg = np.zeros(len(ranges), CK_RANGE)
        rg["first"], rg["count"] = [r[0] for r in ranges], [r[1] for r in ranges]
        out = np.zeros(len(rg), CK_PACK)
        hi = hl = he = hr = None
        if hdr is not None:
            hi = (ctypes.c_void_p * 2)(*hdr[0])
            hl = (ctypes.c_void_p * 2)(*hdr[1])
            he = (ctypes.c_uint64 * 2)(*hdr[2])
            rec = np.array(hdr[3], CK_HDR)
            hr = rec.ctypes.data
        return L.rcdc_check_packs(ctx, d_ids, strides[0], off, strides[1], ln, strides[2], ul,
                                  strides[3], None, count, rg.ctypes.data, len(rg), hi, hl, he, hr,
                                  out.ctypes.data if packs else None, findings[0], findings[1], None,
                                  ctypes.byref(result) if result is not None else None, 0)
    assert call() == 0
    bad = [dict(ctx=None), dict(result=None), dict(d_ids=None), dict(off=None), dict(ln=None),
           dict(ul=None), dict(packs=False), dict(findings=(None, 4)),
           dict(ranges=((0, 4), (5, 4))),                  # a range past n
           dict(ranges=((6, 0xFFFFFFFF),)),
           dict(ranges=((0, 5), (4, 4))),                  # overlapping ranges
           dict(ranges=((2, 2), (0, 3))),
           dict(off=locs.data_ptr() + 5), dict(ln=locs.data_ptr() + 9),   # unaligned arrays
           dict(ul=locs.data_ptr() + 13), dict(strides=(32, 16, 18, 16)),
           dict(strides=(31, 16, 16, 16)), dict(strides=(32, 2, 16, 16)),
           dict(count=0xFFFFFFFF),
           # a header range past its array, a null or unaligned header array, a type above 1
           dict(hdr=((ids.data_ptr(), 0), (locs.data_ptr(), 0), (8, 0), [(0, 4, 5), (0, 4, 0)])),
           dict(hdr=((ids.data_ptr(), 0), (locs.data_ptr(), 0), (8, 0), [(1, 4, 0), (0, 4, 0)])),
           dict(hdr=((ids.data_ptr() + 8, 0), (locs.data_ptr(), 0), (7, 0), [(0, 4, 0), (0, 4, 0)])),
           dict(hdr=((ids.data_ptr(), 0), (locs.data_ptr(), 0), (8, 0), [(2, 4, 0), (0, 4, 0)]))]
    for kw in bad:
        assert call(**kw) == 2, kw   # RCDC_ERR_INVALID_INPUT
        assert b"rcdc_check_packs" in L.rcdc_last_error()
    assert call(hdr=((ids.data_ptr(), 0), (locs.data_ptr(), 0), (8, 0),
                     [(0, 4, 4), (0xFFFFFFFF, 9, 9)])) == 0
    assert call(ranges=()) == 0 and call(count=0, ranges=((0, 0),), d_ids=None) == 0
