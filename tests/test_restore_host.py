"""CPU: the host half of restore (rustic_core_amd/restore.py) -- the read
coalescing of BlobLocations::can_coalesce / append (blob.rs:185-196, with the
cases of its own test, blob.rs:216-225), PackInfo::coalesce and the `packs`
vector of restore_contents (restore.rs:494-508, 561-583), to_packs
(:843-851), the index lookup (repository.rs:1347-1359), data_length
(blob.rs:146-151) -- and rcdc_place_blobs' ABI without a device."""
import ctypes

import pytest

from rustic_core_amd.errors import ErrorKind, RusticError
from rustic_core_amd.index import IndexBlob, IndexFile, IndexPack
from rustic_core_amd.restore import (BlobLocation, FileLocation, PackRead, RestorePlan,
                                     can_coalesce, coalesce, data_length, index_lookup)

KIB, MIB = 1 << 10, 1 << 20
LIMIT = 40 * MIB

COALESCE = [
    (123, 135, 123, 246),
    (123, 135 + 256 * KIB, 123, 246 + 256 * KIB),
    (123, 136 + 256 * KIB, 123, None),
    (LIMIT - 15, LIMIT - 3, 15, LIMIT),
    (LIMIT - 15, LIMIT - 3, 16, None),
    (LIMIT - 15, LIMIT, 12, LIMIT),
    (LIMIT - 15, LIMIT + 1, 12, None),
    (123, 134, 123, None),  # other starts before self ends
    (123, 12, 50, None),
]


@pytest.mark.parametrize("l1,o2,l2,want", COALESCE)
def test_coalesce_boundaries(l1, o2, l2, want):
    a = PackRead(b"p", None, 12, l1, [(BlobLocation(12, l1), [(0, 0)])])
    b = PackRead(b"p", None, o2, l2, [(BlobLocation(o2, l2), [(1, 7)])])
    assert can_coalesce(12, l1, o2, l2) == (want is not None)
    m = coalesce(a, b)
    if want is None:
        assert m is None
    else:
        assert (m.pack_id, m.from_file, m.offset, m.length) == (b"p", None, 12, want)
        assert m.blobs == a.blobs + b.blobs


def _plan(entries):
    p = RestorePlan()
    for key, fls in entries:
        p.r[key] = [FileLocation(*f) for f in fls]
    return p


def test_pack_reads_hand_made_plan():
    A, B = b"\x01" * 32, b"\x02" * 32
    Q = 400 * KIB  # past the hole limit from the first read
    plan = _plan([
        # inserted out of order: the reads come out by pack id, then offset
        ((B, 0, 100, 0), [(0, 0, False)]),
        ((A, 1000, 100, 0), [(1, 68, True), (2, 0, False)]),   # right with from_file: merges
        ((A, 0, 100, 300), [(0, 100, False), (1, 0, False)]),
        ((A, 100, 100, 0), [(0, 400, False)]),
        ((A, Q, 50, 0), [(3, 0, True), (4, 0, False)]),        # left with from_file ...
        ((A, Q + 50, 50, 0), [(4, 18, False)]),                # ... does not merge
        ((A, Q + 100, 60, 0), [(5, 0, True), (6, 0, True)]),   # all match: no destination
        ((A, Q + 160 + 256 * KIB + 1, 40, 0), [(7, 0, False)]),   # past the hole limit
    ])
    reads = plan.pack_reads()
    assert [(r.pack_id, r.from_file, r.offset, r.length) for r in reads] == [
        (A, None, 0, 1100),
        (A, (3, 0, 18), Q, 50),
        (A, None, Q + 50, 110),
        (A, None, Q + 160 + 256 * KIB + 1, 40),
        (B, None, 0, 100),
    ]
    assert reads[0].blobs == [
        (BlobLocation(0, 100, 300), [(0, 100), (1, 0)]),
        (BlobLocation(100, 100, 0), [(0, 400)]),
        (BlobLocation(1000, 100, 0), [(2, 0)]),   # its from_file is dropped, as append does
    ]
    assert reads[1].blobs == [(BlobLocation(Q, 50, 0), [(4, 0)])]
    assert reads[2].blobs == [(BlobLocation(Q + 50, 50, 0), [(4, 18)]),
                              (BlobLocation(Q + 100, 60, 0), [])]
    # two packs never merge although B's offsets would fit
    assert reads[-1].pack_id == B and reads[-2].pack_id == A


def test_pack_reads_order_uncompressed_none_first():
    A = b"\x01" * 32
    plan = _plan([((A, 0, 50, 7), [(0, 0, False)]), ((A, 0, 50, 0), [(1, 0, False)]),
                  ((A, 0, 40, 9), [(2, 0, False)])])
    assert [k for k, _ in plan.restore_info()] == [(A, 0, 40, 9), (A, 0, 50, 0), (A, 0, 50, 7)]


def test_to_packs():
    A, B, C = b"\x01" * 32, b"\x02" * 32, b"\x03" * 32
    plan = _plan([
        ((A, 0, 100, 0), [(0, 0, False)]),
        ((A, 100, 100, 0), [(0, 68, False), (1, 0, False)]),
        ((B, 0, 100, 0), [(0, 136, True)]),
        ((B, 100, 100, 0), [(1, 68, False), (2, 0, True)]),
        ((C, 0, 100, 0), [(3, 0, False)]),
    ])
    assert plan.to_packs() == [A, C]
    assert _plan([((B, 0, 100, 0), [(0, 0, True)]), ((B, 100, 100, 0), [(0, 68, False)]),
                  ((B, 300, 100, 0), [(0, 136, False)])]).to_packs() == [B]


def test_index_lookup():
    i1, i2, i3 = b"\x11" * 32, b"\x22" * 32, b"\x33" * 32
    P1, P2, P3 = b"\xa1" * 32, b"\xa2" * 32, b"\xa3" * 32
    f1 = IndexFile([IndexPack(P1, [IndexBlob(i1, 0, 0, 100, None), IndexBlob(i2, 0, 100, 90, 500)])],
                   [IndexPack(P3, [IndexBlob(i3, 0, 0, 77, None)])])
    f2 = IndexFile([IndexPack(P2, [IndexBlob(i1, 0, 40, 100, None)])])
    idx = index_lookup([f1, f2])
    assert set(idx) == {i1, i2}                      # packs_to_delete is ignored
    assert idx[i1] == (P1, f1.packs[0].blobs[0])     # the first entry wins
    assert idx[i2][0] == P1 and idx[i2][1].uncompressed_length == 500
    plan = RestorePlan()
    with pytest.raises(RusticError) as e:
        plan.add_file("f", 77, [i3], idx)
    assert e.value.kind == ErrorKind.Internal
    assert e.value.message == f"Blob ID `{i3.hex()}` not found in index, but should be there."
    assert plan.names == [] and plan.r == {}
    # without an existing file the plan needs no device
    assert plan.add_file("g", 568, [i1, i2, i1], idx) == "Modify"
    assert plan.file_lengths == [68 + 500 + 68] and plan.restore_size == 636
    assert plan.matched_size == 0
    assert plan.r[(P1, 0, 100, 0)] == [FileLocation(0, 0, False), FileLocation(0, 568, False)]
    assert plan.r[(P1, 100, 90, 500)] == [FileLocation(0, 68, False)]


def test_data_length():
    assert data_length(IndexBlob(b"", 0, 0, 100, None)) == 68
    assert data_length(IndexBlob(b"", 0, 0, 100, 4096)) == 4096
    assert data_length(BlobLocation(5, 32)) == 0
    assert data_length(BlobLocation(5, 40, 9)) == 9


def test_place_blobs_abi(rcdc_lib):
    """rcdc_place_blobs without a GPU: a null context is InvalidInput before
    any HIP call; the ctypes structs have the header's sizes."""
    from rustic_core_amd import _lib
    from rustic_core_amd.pack import PLACE_BLOB, PLACE_DEST, PlaceBlob, PlaceDest
    assert ctypes.sizeof(PlaceBlob) == 32 and ctypes.sizeof(PlaceDest) == 16
    assert PLACE_BLOB.itemsize == 32 and PLACE_DEST.itemsize == 16
    assert [f[0] for f in PlaceBlob._fields_] == list(PLACE_BLOB.names)
    assert [f[0] for f in PlaceDest._fields_] == list(PLACE_DEST.names)
    L = _lib.lib()
    assert L.rcdc_place_blobs(None, None, None, 0, None, 0, None, 0, None, None, 0, 0, None,
                              None) == 2
    assert "ctx is NULL" in _lib.last_error()
    assert rcdc_lib.rcdc_abi_version() == 5
