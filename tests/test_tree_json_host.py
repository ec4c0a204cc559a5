"""CPU: the grammar G_T of rcdc_tree_parse (include/rcdc.h) -- the model judges
the case table as the table says, ``tree.parse_tree_host`` agrees with the
model's ``ids_of``, and the library's bound and argument checks hold without
a device."""
import ctypes
import json
import random

import pytest

from tests import tree_json_model as model
from tests.index_json_cases import hid
from tests.tree_json_cases import CASES, flipped, random_text, random_tree

SYMBOLS = ("rcdc_tree_parse", "rcdc_tree_parse_bound", "rcdc_tree_parse_tile")


@pytest.mark.parametrize("name,data,in_gt", CASES, ids=[c[0] for c in CASES])
def test_model_judges_the_table(name, data, in_gt):
    assert model.in_gt(data) == in_gt


def test_table_has_every_rule():
    names = {c[0] for c in CASES}
    assert len([c for c in CASES if c[2]]) >= 25 and len([c for c in CASES if not c[2]]) >= 60
    for want in ("rustic_style", "restic_style", "every_node_type", "content_null", "content_absent",
                 "content_empty", "non_dir_with_subtree", "nodes_null", "keys_permuted_0",
                 "every_whitespace", "name_escaped_quote", "name_escaped_backslash",
                 "name_backslash_then_quote", "name_unicode_escape", "name_utf8_2_3_4_bytes",
                 "name_is_content_user_is_subtree", "xattr_named_content",
                 "duplicate_content", "unknown_key", "escaped_key", "id_63_digits", "id_65_digits",
                 "id_not_hex", "id_with_escape", "unknown_type", "symlink_without_linktarget",
                 "dir_without_subtree", "mode_two_pow_32", "leading_zero", "negative_number",
                 "raw_control_byte_in_name", "bad_escape", "escape_ud800", "utf8_overlong_2",
                 "utf8_truncated", "unclosed_string", "depth_6", "second_root_key",
                 "trailing_non_whitespace"):
        assert want in names, want


def _is_json(data: bytes) -> bool:
    try:
        json.loads(data.decode("utf-8"))
        return True
    except ValueError:
        return False


def test_parse_tree_host_against_the_model():
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.tree import DESERIALIZE_MESSAGE, parse_tree_host
    not_json = 0
    for name, data, in_gt in CASES:
        if in_gt:
            assert parse_tree_host(data) == model.ids_of(data), name
        elif not _is_json(data):
            not_json += 1
            with pytest.raises(RusticError) as e:
                parse_tree_host(data)
            assert e.value.kind == ErrorKind.Internal and DESERIALIZE_MESSAGE in str(e.value), name
    assert not_json >= 30
    # outside G_T, still a tree for the host: an unknown key, an escape in an id and in a key
    by_name = {c[0]: c[1] for c in CASES}
    for name in ("unknown_key", "unknown_key_null", "id_with_escape", "escaped_key",
                 "escape_surrogate_pair", "type_with_escape"):
        assert not model.in_gt(by_name[name])
        assert parse_tree_host(by_name[name]) == model.ids_of(by_name[name]), name
    # ... and what Node's deserialiser refuses although it is JSON
    for name in ("id_63_digits", "id_not_hex", "id_is_null", "unknown_type", "type_absent",
                 "name_absent", "symlink_without_linktarget", "dir_without_subtree",
                 "mode_two_pow_32", "negative_number", "duplicate_content", "node_is_number",
                 "root_empty_object", "root_is_array"):
        with pytest.raises(RusticError):
            parse_tree_host(by_name[name])


def test_random_trees_are_in_gt():
    from rustic_core_amd.tree import parse_tree_host
    rng = random.Random(3)
    kept = 0
    for _ in range(300):
        text = random_text(random_tree(rng), rng)
        assert model.in_gt(text)
        assert parse_tree_host(text) == model.ids_of(text)
        bad = flipped(text, rng)
        if model.in_gt(bad):
            kept += 1
            assert parse_tree_host(bad) == model.ids_of(bad)
    assert 0 < kept < 300  # a flip may leave a blob inside G_T: the model decides


# ---- the ABI without a device ---------------------------------------------------

def test_symbols_and_structs(rcdc_lib):
    from rustic_core_amd import _lib
    from rustic_core_amd.tree import TR_BLOB, TR_REF, parse_tile
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    assert TR_REF.itemsize == 16 and TR_BLOB.itemsize == 32
    assert ctypes.sizeof(_lib.TrparseResult) == 32
    assert parse_tile() >= 1024 and parse_tile() % 1024 == 0


def test_bound_against_the_densest_blobs(rcdc_lib):
    from rustic_core_amd.tree import parse_bound
    one_id = b'"' + hid(1).encode() + b'"'
    sub_node = b'{"name":"","type":"dir","subtree":' + one_id + b"}"
    small_node = b'{"name":"","type":"dev"}'
    assert len(one_id) == 66 and len(sub_node) == 101 and len(small_node) == 24
    for n in (1, 2, 3, 50, 4097):
        ids = b",".join([one_id] * n)
        assert parse_bound(len(ids))[0] == n and parse_bound(len(ids) - 1)[0] == n - 1
        subs = b",".join([sub_node] * n)
        assert parse_bound(len(subs))[1] == n and parse_bound(len(subs) - 1)[1] == n - 1
        nodes = b",".join([small_node] * n)
        assert parse_bound(len(nodes))[2] == n and parse_bound(len(nodes) - 1)[2] == n - 1
        # whole blobs of the densest kind are in G_T and within the bound
        f1 = b'{"nodes":[{"name":"","type":"file","content":[' + ids + b"]}]}"
        f2 = b'{"nodes":[' + subs + b"]}"
        f3 = b'{"nodes":[' + nodes + b"]}"
        for f, nn, nd, nt in ((f1, 1, n, 0), (f2, n, 0, n), (f3, n, 0, 0)):
            assert model.in_gt(f)
            got = model.ids_of(f)
            assert (got[0], len(got[1]), len(got[2])) == (nn, nd, nt)
            b = parse_bound(len(f))
            assert b[0] >= nd and b[1] >= nt and b[2] >= nn
    assert parse_bound(0) == (0, 0, 0) and parse_bound(66) == (1, 0, 2)
    # no accepted case of the table holds more than its bound
    for name, data, in_gt in CASES:
        if in_gt:
            nn, d, t = model.ids_of(data)
            b = parse_bound(len(data))
            assert len(d) <= b[0] and len(t) <= b[1] and nn <= b[2], name


def test_refused_before_any_hip_call(rcdc_lib):
    """Null and out-of-range arguments are InvalidInput with no device: the
    context is a dummy that is never dereferenced on these paths."""
    from rustic_core_amd import _lib
    from rustic_core_amd.tree import TR_BLOB
    import numpy as np
    L = rcdc_lib
    res = _lib.TrparseResult()
    n_text = 67 * 4  # bound: 4 content ids, 2 subtrees
    refs = (_lib.IxparseRef * 1)(_lib.IxparseRef(0, n_text))  # rcdc_trparse_ref has the same layout
    blobs = np.zeros(1, TR_BLOB)
    fake = ctypes.c_void_p(64)  # stands for device memory / a context; never read
    r, b, rs = ctypes.addressof(refs), blobs.ctypes.data, ctypes.byref(res)

    def call(ctx=fake, text=fake, text_len=n_text, refs_=r, n=1, data=fake, cap_d=4, tree=fake,
             is_dir=fake, cap_t=2, blobs_=b, res_=rs):
        return L.rcdc_tree_parse(ctx, text, text_len, refs_, n, data, cap_d, tree, is_dir, cap_t,
                                 blobs_, res_, None)
    assert call(ctx=None) == 2 and "ctx is NULL" in _lib.last_error()
    assert call(ctx=None, n=0, refs_=None) == 2
    assert call(res_=None) == 2
    for kw in ({"refs_": None}, {"blobs_": None}, {"text": None}):
        assert call(**kw) == 2, kw
    # a ref outside the arena
    assert call(text_len=n_text - 1) == 2 and "outside the arena" in _lib.last_error()
    refs[0].off = 1
    assert call() == 2
    refs[0].off = 2 ** 64 - 1
    assert call() == 2
    refs[0].off = 0
    # capacities below the bound
    assert call(cap_d=3) == 2 and "below" in _lib.last_error()
    assert call(cap_t=1) == 2 and "below" in _lib.last_error()
    assert call(cap_t=1, tree=None) == 2  # the flags alone need the capacity too
    # misaligned id arrays
    assert call(data=ctypes.c_void_p(72)) == 2 and "aligned" in _lib.last_error()
    assert call(tree=ctypes.c_void_p(72)) == 2
    # n == 0 launches nothing: fine without arrays (the context is not touched)
    res.blobs_not_parsed = 7
    assert L.rcdc_tree_parse(fake, None, 0, None, 0, None, 0, None, None, 0, None, rs, None) == 0
    assert res.blobs_not_parsed == 0 and res.data_ids == 0
