"""CPU: rcdc_dindex's ABI without a device -- the symbols, the struct sizes,
what is refused before any HIP call -- and DeviceIndex's argument checks
(rustic_core_amd/dindex.py), which come before the first device call."""
import ctypes

import numpy as np
import pytest

from rustic_core_amd.errors import ErrorKind, RusticError

SYMBOLS = ("rcdc_dindex_create", "rcdc_dindex_destroy", "rcdc_dindex_size", "rcdc_dindex_keys",
           "rcdc_dindex_add", "rcdc_dindex_lookup", "rcdc_dindex_first_new")


def test_symbols_and_structs(rcdc_lib):
    from rustic_core_amd import _lib
    from rustic_core_amd.dindex import HIT, LOC
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    assert ctypes.sizeof(_lib.DindexLoc) == 16 and ctypes.sizeof(_lib.DindexHit) == 24
    assert LOC.itemsize == 16 and HIT.itemsize == 24
    assert [f[0] for f in _lib.DindexLoc._fields_] == list(LOC.names)
    assert [f[0] for f in _lib.DindexHit._fields_][:2] == list(HIT.names[:2])
    assert list(HIT.names[2:]) == list(LOC.names)
    assert rcdc_lib.rcdc_abi_version() == 5


def test_null_index_is_invalid_input(rcdc_lib):
    """A null index or context is InvalidInput before any HIP call, also
    with n == 0 and null arrays: the index is checked first."""
    from rustic_core_amd import _lib
    L = rcdc_lib
    out = ctypes.c_void_p()
    assert L.rcdc_dindex_create(None, 0, ctypes.byref(out)) == 2
    assert "ctx is NULL" in _lib.last_error()
    assert out.value is None
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    for n, a in ((0, None), (1, p)):
        assert L.rcdc_dindex_add(None, a, None, n, 0, None) == 2
        assert "index is NULL" in _lib.last_error()
        assert L.rcdc_dindex_add(None, a, a, n, 1, None) == 2
        assert L.rcdc_dindex_lookup(None, a, n, a, None) == 2
        assert "index is NULL" in _lib.last_error()
        assert L.rcdc_dindex_first_new(None, a, n, None, a, None) == 2
        assert "index is NULL" in _lib.last_error()
    assert L.rcdc_dindex_size(None) == 0 and L.rcdc_dindex_keys(None) == 0
    L.rcdc_dindex_destroy(None)  # a no-op


def test_device_index_argument_checks():
    """Shapes, dtypes and types are refused before a device is needed."""
    from rustic_core_amd import DeviceIndex, IndexType
    from rustic_core_amd.dindex import DATA, TREE
    dx = DeviceIndex(0, IndexType.FULL)
    bad_ids = [np.zeros((4, 31), np.uint8), np.zeros((4, 32), np.int8), np.zeros(32, np.uint8),
               np.zeros((2, 2, 32), np.uint8), [b"\0" * 32], None]
    for ids in bad_ids:
        for call in (lambda: dx.lookup(DATA, ids), lambda: dx.has(TREE, ids),
                     lambda: dx.count_used(DATA, ids), lambda: dx.first_new(ids),
                     lambda: dx.add_ids(ids)):
            with pytest.raises(RusticError) as e:
                call()
            assert e.value.kind == ErrorKind.InvalidInput
    ok = np.zeros((1, 32), np.uint8)
    for tpe in (2, -1, "data", None, True):
        for call in (lambda: dx.lookup(tpe, ok), lambda: dx.has(tpe, ok),
                     lambda: dx.has(tpe, b"\0" * 32), lambda: dx.get_id(tpe, b"\0" * 32),
                     lambda: dx.entries(tpe, []), lambda: dx.total_size(tpe),
                     lambda: dx.packs(tpe), lambda: dx.count_used(tpe, ok)):
            with pytest.raises(RusticError) as e:
                call()
            assert e.value.kind == ErrorKind.InvalidInput
    with pytest.raises(RusticError) as e:
        dx.get_id(DATA, b"\0" * 31)
    assert e.value.kind == ErrorKind.InvalidInput
    with pytest.raises(RusticError) as e:
        DeviceIndex(0, "Full")
    assert e.value.kind == ErrorKind.InvalidInput
    # nothing was added and no device index was made
    assert len(dx) == 0 and dx.total_size(DATA) == 0 and dx.packs(TREE) == []


def test_extend_host_side_without_entries():
    """ONLY_TREES keeps a data pack's id and size and none of its entries,
    so nothing goes to the device."""
    from rustic_core_amd import DeviceIndex, IndexType
    from rustic_core_amd.dindex import DATA, TREE
    from rustic_core_amd.index import IndexBlob, IndexPack
    p = IndexPack(b"\xa1" * 32, [IndexBlob(b"\x11" * 32, 0, 0, 100, None),
                                 IndexBlob(b"\x22" * 32, 0, 100, 90, 500)])
    empty = IndexPack(b"\xa2" * 32, [], size=77)
    dx = DeviceIndex(0, IndexType.ONLY_TREES)
    dx.extend([p, empty])
    assert dx.packs(DATA) == [p.id, empty.id] and dx.packs(TREE) == []
    assert dx.total_size(DATA) == p.pack_size() + 77 == 100 + 90 + 37 + 41 + 36 + 77
    assert dx.total_size(TREE) == 0 and len(dx) == 0
    assert dx.get_id(DATA, b"\x11" * 32) is None
