"""CPU: the grammar G of rcdc_index_parse and its ABI without a device.

The model (tests/index_json_model.py) is checked against the hand-built table
(tests/index_json_cases.py) and, on every file in G, against today's host
path: ``IndexFile.from_json`` followed by ``DeviceIndex.extend``, whose
bookkeeping is replayed with the device add captured.  Then the symbols, the
struct sizes, what is refused before any HIP call, and the bound function."""
import ctypes
import random

import numpy as np
import pytest

from tests import index_json_model as model
from tests.index_json_cases import CASES, ONE_BLOB, compact, hid, random_index, random_text

SYMBOLS = ("rcdc_index_parse", "rcdc_index_parse_bound", "rcdc_index_parse_tile")


def host_collect(files, index_type=None):
    """from_json + extend over ``files`` with the device add captured:
    (packs per type, total size per type, ids per type, locs per type)."""
    from rustic_core_amd import DeviceIndex, IndexType
    from rustic_core_amd.dindex import DATA, TREE
    from rustic_core_amd.index import IndexFile
    dx = DeviceIndex(0, index_type or IndexType.FULL)
    ids, locs = {DATA: [], TREE: []}, {DATA: [], TREE: []}

    def capture(t, a, l, flags):
        tpe = DATA if t is dx._t[DATA] else TREE
        ids[tpe] += [bytes(r) for r in a]
        if l is not None:
            locs[tpe] += [tuple(int(x) for x in r) for r in l.tolist()]
    dx._add = capture
    for data in files:
        dx.extend(IndexFile.from_json(data).packs)
    return ({t: dx.packs(t) for t in (DATA, TREE)}, {t: dx.total_size(t) for t in (DATA, TREE)},
            ids, locs)


def assert_model_is_extend(files):
    packs, total, ids, locs = host_collect(files)
    m = model.collect(files)
    assert m.status == [0] * len(files)
    for t in (0, 1):
        assert [p[0] for p in m.packs if p[1] == t] == packs[t]
        assert [p[2] for p in m.packs if p[1] == t] == list(range(len(packs[t])))
        assert sum(p[3] for p in m.packs if p[1] == t) == total[t]
        assert m.ids[t] == ids[t]
        assert m.locs[t] == locs[t]


@pytest.mark.parametrize("name,data,in_g", CASES, ids=[c[0] for c in CASES])
def test_model_verdict_is_the_table(name, data, in_g):
    assert (model.parse(data) is not None) == in_g


def test_table_covers_both_sides():
    assert sum(1 for c in CASES if c[2]) >= 25 and sum(1 for c in CASES if not c[2]) >= 60


@pytest.mark.parametrize("name,data", [(c[0], c[1]) for c in CASES if c[2]],
                         ids=[c[0] for c in CASES if c[2]])
def test_g_is_a_subset_of_from_json(name, data):
    """On a file in G, from_json succeeds and extend keeps what the model
    collects (packs_to_delete counted only)."""
    from rustic_core_amd.index import IndexFile
    f = IndexFile.from_json(data)
    packs, ndel = model.parse(data)
    assert len(f.packs_to_delete) == ndel and len(f.packs) == len(packs)
    assert_model_is_extend([data])


def test_table_as_one_batch():
    """Pack numbers run on over the files of a batch; files outside G add
    nothing and shift nothing."""
    good = [c[1] for c in CASES if c[2]]
    assert_model_is_extend(good)
    m_all = model.collect([c[1] for c in CASES], (3, 5))
    m_good = model.collect(good, (3, 5))
    assert m_all.packs == m_good.packs and m_all.locs == m_good.locs and m_all.ids == m_good.ids
    assert m_all.status == [0 if c[2] else 1 for c in CASES]


def test_random_files():
    rng = random.Random(20240607)
    files = []
    for k in range(40):
        f = random_index(rng, rng.randrange(6), 12)
        text = random_text(f, rng)
        assert model.parse(text) is not None, k
        assert model.parse(f.to_json()) is not None, k
        files += [text, f.to_json()]
    assert_model_is_extend(files)


def test_only_trees_and_data_ids_keep_what_the_model_says():
    from rustic_core_amd import IndexType
    files = [c[1] for c in CASES if c[2]]
    m = model.collect(files)
    for it in (IndexType.DATA_IDS, IndexType.ONLY_TREES):
        packs, total, ids, locs = host_collect(files, it)
        for t in (0, 1):
            assert [p[0] for p in m.packs if p[1] == t] == packs[t]
            assert sum(p[3] for p in m.packs if p[1] == t) == total[t]
        assert ids[1] == m.ids[1] and locs[1] == m.locs[1]
        assert ids[0] == ([] if it == IndexType.ONLY_TREES else m.ids[0]) and locs[0] == []


# ---- the ABI without a device ---------------------------------------------------

def test_symbols_and_structs(rcdc_lib):
    from rustic_core_amd import _lib
    from rustic_core_amd.dindex import IX_FILE, IX_PACK, IX_REF
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    assert ctypes.sizeof(_lib.IxparseRef) == IX_REF.itemsize == 16
    assert ctypes.sizeof(_lib.IxparseFile) == IX_FILE.itemsize == 24
    assert ctypes.sizeof(_lib.IxparsePack) == IX_PACK.itemsize == 48
    assert ctypes.sizeof(_lib.IxparseResult) == 40
    assert [f[0] for f in _lib.IxparseFile._fields_] == list(IX_FILE.names)
    assert [f[0] for f in _lib.IxparsePack._fields_] == list(IX_PACK.names)
    assert rcdc_lib.rcdc_abi_version() == 5
    tile = rcdc_lib.rcdc_index_parse_tile()
    assert tile >= 1024 and tile % 1024 == 0


def test_bound_against_the_smallest_objects(rcdc_lib):
    from rustic_core_amd.dindex import parse_bound
    small_blob = b'{"id":"' + hid(1).encode() + b'","type":"data","offset":0,"length":0}'
    small_pack = b'{"id":"' + hid(2).encode() + b'","blobs":[]}'
    assert len(small_blob) == 109 and len(small_pack) == 84
    for n in (1, 2, 3, 50):
        blobs = b",".join([small_blob] * n)
        assert parse_bound(len(blobs)) [0] == n and parse_bound(len(blobs) - 1)[0] == n - 1
        packs = b",".join([small_pack] * n)
        assert parse_bound(len(packs))[1] == n and parse_bound(len(packs) - 1)[1] == n - 1
        # whole files of smallest objects are in G and within the bound
        f1 = b'{"packs":[{"id":"' + hid(2).encode() + b'","blobs":[' + blobs + b"]}]}"
        f2 = b'{"packs":[' + packs + b"]}"
        for f, ne, npk in ((f1, n, 1), (f2, 0, n)):
            got = model.parse(f)
            assert got is not None and len(got[0]) == npk and sum(len(p[1]) for p in got[0]) == ne
            assert parse_bound(len(f))[0] >= ne and parse_bound(len(f))[1] >= npk
    assert parse_bound(0) == (0, 0) and parse_bound(108) == (0, 1)
    # no accepted case of the table holds more than its bound
    for name, data, in_g in CASES:
        if in_g:
            packs, ndel = model.parse(data)
            assert sum(len(p[1]) for p in packs) <= parse_bound(len(data))[0], name
            assert len(packs) + ndel <= parse_bound(len(data))[1], name


def test_refused_before_any_hip_call(rcdc_lib):
    """Null and out-of-range arguments are InvalidInput with no device: the
    context is a dummy that is never dereferenced on these paths."""
    from rustic_core_amd import _lib
    L = rcdc_lib
    res = _lib.IxparseResult()
    text = ONE_BLOB
    refs = (_lib.IxparseRef * 1)(_lib.IxparseRef(0, len(text)))
    files = (_lib.IxparseFile * 1)()
    packs = (_lib.IxparsePack * 4)()
    base = (ctypes.c_uint32 * 2)(0, 0)
    two = (ctypes.c_void_p * 2)(None, None)
    fake = ctypes.c_void_p(64)  # stands for device memory / a context; never read
    r, f, p, b, t = (ctypes.addressof(x) for x in (refs, files, packs, base, two))
    rs = ctypes.byref(res)

    def call(ctx=fake, json=fake, json_len=len(text), refs_=r, n=1, base_=b, ids=t, locs=t,
             cap_e=1, files_=f, packs_=p, cap_p=4, res_=rs):
        return L.rcdc_index_parse(ctx, json, json_len, refs_, n, base_, ids, locs, cap_e, files_,
                                  packs_, cap_p, res_, None)
    assert call(ctx=None) == 2 and "ctx is NULL" in _lib.last_error()
    assert call(ctx=None, n=0, refs_=None) == 2
    assert call(res_=None) == 2
    for kw in ({"refs_": None}, {"files_": None}, {"base_": None}, {"ids": None}, {"locs": None},
               {"packs_": None}, {"json": None}):
        assert call(**kw) == 2, kw
    # a ref outside the arena
    assert call(json_len=len(text) - 1) == 2 and "outside the arena" in _lib.last_error()
    refs[0].off = 1
    assert call() == 2
    refs[0].off = 2 ** 64 - 1
    assert call() == 2
    refs[0].off = 0
    # capacities below the bound
    assert call(cap_e=0) == 2 and "below" in _lib.last_error()
    assert call(cap_p=0) == 2
    # misaligned entry arrays
    odd = (ctypes.c_void_p * 2)(72, None)
    assert call(ids=ctypes.addressof(odd)) == 2
    # n == 0 launches nothing: fine without arrays (the context is not touched)
    res.files_not_parsed = 7
    assert L.rcdc_index_parse(fake, None, 0, None, 0, None, None, None, 0, None, None, 0, rs,
                              None) == 0
    assert res.files_not_parsed == 0 and res.packs[0] == 0


def test_python_argument_checks():
    from rustic_core_amd.dindex import _frame_content_size, _BAD
    magic = b"\x28\xb5\x2f\xfd"
    assert _frame_content_size(magic + b"\x20\x05") == 5          # single segment, 1 byte
    assert _frame_content_size(magic + b"\x60\x05\x01") == 0x105 + 256
    assert _frame_content_size(magic + b"\x00\x58") is None       # window only, no size
    assert _frame_content_size(magic + b"\x80\x58\x01\x02\x03\x04") == 0x04030201
    assert _frame_content_size(magic + b"\x80\x58\x01") is _BAD   # header cut short
    assert _frame_content_size(b"\x28\xb5\x2f\xfc\x00\x58") is _BAD
    assert _frame_content_size(b"") is _BAD
    assert compact({"a": 1}) == b'{"a":1}'
