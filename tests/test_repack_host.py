"""CPU: the host half of repack and copy (rustic_core_amd/repack.py) --
CopyPackBlobs::coalesce (packer.rs:896-905, with the cases of blob.rs:216-225
that tests/test_restore_host.py uses), copy_blobs' sorted and coalesced plan
(copy.rs:150-159) and the per-pack plan of prune's repack
(prune.rs:1320-1323, :1408-1417)."""
import pytest

from rustic_core_amd.index import IndexBlob, IndexPack
from rustic_core_amd.repack import CopyPackBlobs, plan_copy, plan_repack
from rustic_core_amd.restore import BlobLocation, can_coalesce
from tests.test_restore_host import COALESCE, KIB

A, B = b"\x01" * 32, b"\x02" * 32


def _id(k: int) -> bytes:
    return bytes([k]) * 32


@pytest.mark.parametrize("l1,o2,l2,want", COALESCE)
def test_coalesce_boundaries(l1, o2, l2, want):
    a = CopyPackBlobs(A, 12, l1, [(BlobLocation(12, l1), _id(1))])
    b = CopyPackBlobs(A, o2, l2, [(BlobLocation(o2, l2, 9), _id(2))])
    assert can_coalesce(12, l1, o2, l2) == (want is not None)
    m = a.coalesce(b)
    assert m == CopyPackBlobs.coalesce(a, b)
    if want is None:
        assert m is None
    else:
        assert (m.pack_id, m.offset, m.length) == (A, 12, want)
        assert m.blobs == a.blobs + b.blobs
    # another pack never merges
    assert a.coalesce(CopyPackBlobs(B, o2, l2, b.blobs)) is None


def test_from_index_entry():
    c = CopyPackBlobs.from_index_entry(A, IndexBlob(_id(7), 1, 40, 100, 555))
    assert c == CopyPackBlobs(A, 40, 100, [(BlobLocation(40, 100, 555), _id(7))])
    c = CopyPackBlobs.from_index_entry(A, IndexBlob(_id(8), 0, 0, 33, None))
    assert c.blobs == [(BlobLocation(0, 33, 0), _id(8))]


def test_plan_copy_sorts_and_coalesces():
    Q = 400 * KIB  # past the hole limit from the first read
    entries = [
        # out of order: the reads come out by pack id, then offset
        (B, IndexBlob(_id(1), 0, 0, 100, None)),
        (A, IndexBlob(_id(2), 0, 1000, 100, None)),       # a hole of 800: merges
        (A, IndexBlob(_id(3), 0, 0, 100, 300)),
        (A, IndexBlob(_id(4), 0, 100, 100, None)),
        (A, IndexBlob(_id(5), 0, Q, 50, 70)),
        (A, IndexBlob(_id(6), 0, Q + 50, 50, None)),
        (A, IndexBlob(_id(7), 0, Q + 100 + 256 * KIB + 1, 40, None)),   # past the hole limit
        (B, IndexBlob(_id(8), 0, 100, 60, None)),
    ]
    plan = plan_copy(iter(entries))
    assert [(c.pack_id, c.offset, c.length) for c in plan] == [
        (A, 0, 1100),
        (A, Q, 100),
        (A, Q + 100 + 256 * KIB + 1, 40),
        (B, 0, 160),
    ]
    assert plan[0].blobs == [(BlobLocation(0, 100, 300), _id(3)), (BlobLocation(100, 100, 0), _id(4)),
                             (BlobLocation(1000, 100, 0), _id(2))]
    assert plan[1].blobs == [(BlobLocation(Q, 50, 70), _id(5)), (BlobLocation(Q + 50, 50, 0), _id(6))]
    assert plan[3].blobs == [(BlobLocation(0, 100, 0), _id(1)), (BlobLocation(100, 60, 0), _id(8))]
    # two packs never merge although B's offsets would fit behind A's
    assert plan_copy([(A, IndexBlob(_id(1), 0, 0, 100, None)),
                      (B, IndexBlob(_id(2), 0, 100, 100, None))]) == [
        CopyPackBlobs(A, 0, 100, [(BlobLocation(0, 100, 0), _id(1))]),
        CopyPackBlobs(B, 100, 100, [(BlobLocation(100, 100, 0), _id(2))])]
    assert plan_copy([]) == []


def test_plan_copy_same_location_twice_does_not_merge():
    """The same blob listed twice (two ids of one location cannot happen, two
    requests for one id can): the second starts before the first ends."""
    e = (A, IndexBlob(_id(1), 0, 0, 100, None))
    plan = plan_copy([e, e])
    assert [(c.offset, c.length, len(c.blobs)) for c in plan] == [(0, 100, 1), (0, 100, 1)]


def test_plan_repack():
    p1 = IndexPack(A, [IndexBlob(_id(4), 0, 300, 100, None), IndexBlob(_id(1), 0, 0, 100, 400),
                       IndexBlob(_id(2), 0, 100, 100, None), IndexBlob(_id(3), 0, 200, 100, None),
                       IndexBlob(_id(5), 0, 400 + 300 * KIB, 64, None)])
    p2 = IndexPack(B, [IndexBlob(_id(3), 0, 0, 100, None), IndexBlob(_id(6), 0, 100, 100, None),
                       IndexBlob(_id(7), 0, 200, 100, None)])
    used = {_id(1), _id(3), _id(4), _id(5), _id(6), _id(99)}
    r1 = plan_repack(p1, used)
    # only used ids, by offset; the unused blob 2 leaves a hole that is read over
    assert r1 == [
        CopyPackBlobs(A, 0, 400, [(BlobLocation(0, 100, 400), _id(1)), (BlobLocation(200, 100, 0), _id(3)),
                                  (BlobLocation(300, 100, 0), _id(4))]),
        CopyPackBlobs(A, 400 + 300 * KIB, 64, [(BlobLocation(400 + 300 * KIB, 64, 0), _id(5))]),
    ]
    assert used == {_id(6), _id(99)}   # the kept ids are taken out of the set
    # blob 3 is in both packs: the first pack kept it, the second does not
    r2 = plan_repack(p2, used)
    assert r2 == [CopyPackBlobs(B, 100, 100, [(BlobLocation(100, 100, 0), _id(6))])]
    assert used == {_id(99)}
    assert plan_repack(p2, used) == [] and used == {_id(99)}
    assert p1.blobs[0].id == _id(4) and len(p1.blobs) == 5   # the index pack is left as it is


def test_public_names():
    import rustic_core_amd as r
    for name in ("BlobCopier", "CopyPackBlobs", "NewPack", "plan_copy", "plan_repack"):
        assert name in r.__all__ and hasattr(r, name)
