"""Hand-built index files for the grammar G of rcdc_index_parse: (name, bytes,
in G?).  The accepted ones cover the forms index files come in; the rejected
ones break one rule of G each.  Also the generator of random valid files."""
import json
import random


def hid(n: int) -> str:
    """A 64-digit id that tells blobs and packs apart by number."""
    return f"{n:02x}" * 8 + f"{(n * 7 + 3) % 256:02x}" * 24


def blob(n, tpe="data", off=0, length=100, ulen=None, keep_ulen=True) -> dict:
    o = {"id": hid(n), "type": tpe, "offset": off, "length": length}
    if keep_ulen:
        o["uncompressed_length"] = ulen
    return o


def compact(o) -> bytes:
    return json.dumps(o, separators=(",", ":")).encode()


def permuted(o, rng):
    """The same value with the keys of every object in another order."""
    if isinstance(o, dict):
        ks = list(o)
        rng.shuffle(ks)
        return {k: permuted(o[k], rng) for k in ks}
    if isinstance(o, list):
        return [permuted(x, rng) for x in o]
    return o


def spaced(o, rng) -> bytes:
    """JSON text with random runs of the four whitespace bytes between any
    two tokens and around the root."""
    ws = lambda: "".join(rng.choice(" \t\n\r") for _ in range(rng.choice((0, 0, 1, 2, 5))))

    def emit(x):
        if isinstance(x, dict):
            return "{" + ws() + ",".join(ws() + json.dumps(k) + ws() + ":" + ws() + emit(v) + ws()
                                         for k, v in x.items()) + "}"
        if isinstance(x, list):
            return "[" + ws() + ",".join(ws() + emit(v) + ws() for v in x) + "]"
        return json.dumps(x)
    return (ws() + emit(o) + ws()).encode()


P1 = {"id": hid(200), "blobs": [blob(1, "data", 0, 100), blob(2, "data", 100, 250, 900)]}
P2 = {"id": hid(201), "blobs": [blob(3, "tree", 0, 77, 300), blob(4, "tree", 77, 1)],
      "time": "2024-05-06T07:08:09.123456789+02:00"}
REF = {"packs": [P1, P2]}
ONE = lambda b, **kw: compact({"packs": [dict({"id": hid(9), "blobs": [b]}, **kw)]})
ONE_BLOB = compact({"packs": [{"id": hid(9), "blobs": [blob(1)]}]})


def _rep(src: bytes, old: bytes, new: bytes) -> bytes:
    assert src.count(old) >= 1, (src, old)
    return src.replace(old, new, 1)


def _cases():
    rng = random.Random(5)
    yes, no = [], []
    yes.append(("reference_compact", compact(REF)))
    yes.append(("restic_form", compact({
        "supersedes": [hid(50), hid(51)],
        "packs": [{"id": hid(9), "blobs": [blob(1, keep_ulen=False), blob(2, "data", 5, 6, 7, True),
                                           blob(3, "data", 9, 4294967295, keep_ulen=False)]}]})))
    yes.append(("supersedes_null_and_empty", compact({"supersedes": None, "packs": [P1]})))
    yes.append(("supersedes_empty", compact({"packs": [P1], "supersedes": []})))
    yes.append(("pretty", json.dumps(REF, indent=2).encode()))
    yes.append(("pretty_tabs_crlf", json.dumps(REF, indent="\t").replace("\n", "\r\n").encode()))
    yes.append(("every_whitespace", spaced(REF, rng)))
    yes.append(("whitespace_around_root", b" \t\r\n" + compact(REF) + b"\n \t\r"))
    for i in range(3):
        yes.append((f"keys_permuted_{i}", compact(permuted(
            {"supersedes": [hid(60)], "packs": [dict(P2, size=5), P1], "packs_to_delete": [P1]}, rng))))
    yes.append(("upper_case_hex", compact(REF).replace(hid(1).encode(), hid(1).upper().encode())
                .replace(hid(200).encode(), hid(200).upper().encode())))
    yes.append(("mixed_case_hex", compact({"packs": [{"id": "aBcDeF" + hid(1)[6:], "blobs": []}]})))
    yes.append(("size_and_time_present", compact({"packs": [dict(P1, time="t", size=12345)]})))
    yes.append(("size_zero", compact({"packs": [dict(P1, size=0)]})))
    yes.append(("size_max", compact({"packs": [dict(P1, size=4294967295)]})))
    yes.append(("size_and_time_null", compact({"packs": [dict(P1, time=None, size=None)]})))
    yes.append(("time_empty_and_odd", compact({"packs": [dict(P1, time=""), dict(P2, time="{[ ]},:~ ")]})))
    yes.append(("packs_to_delete", compact({"packs": [P1], "packs_to_delete": [P2, P1]})))
    yes.append(("packs_to_delete_first", compact({"packs_to_delete": [P2], "packs": [P1]})))
    yes.append(("packs_to_delete_empty", compact({"packs": [P1], "packs_to_delete": []})))
    yes.append(("empty_pack", compact({"packs": [{"id": hid(7), "blobs": []}]})))
    yes.append(("empty_packs_between", compact({"packs": [
        {"id": hid(7), "blobs": []}, P2, {"blobs": [], "id": hid(8), "size": 77}, P1,
        {"id": hid(6), "blobs": []}]})))
    yes.append(("mixed_types_in_a_pack", compact({"packs": [
        {"id": hid(9), "blobs": [blob(1, "tree", 0, 10), blob(2, "data", 10, 20, 30)]},
        {"id": hid(10), "blobs": [blob(3, "data", 0, 10), blob(4, "tree", 10, 20)]}]})))
    yes.append(("empty_packs", compact({"packs": []})))
    yes.append(("empty_packs_spaced", b'{ "packs" : [ ] }'))
    yes.append(("offset_zero_length_zero", ONE(blob(1, "data", 0, 0))))
    yes.append(("ulen_max", ONE(blob(1, "data", 1, 2, 4294967295))))

    no.append(("backslash_in_time", compact({"packs": [dict(P1, time="a\\b")]})))
    no.append(("backslash_escaped_quote", compact({"packs": [dict(P1, time='a"b')]})))
    no.append(("unicode_escape_in_id", _rep(ONE_BLOB, hid(1).encode(), b"\\u0061" + hid(1)[1:].encode())))
    no.append(("id_63_digits", _rep(ONE_BLOB, hid(1).encode(), hid(1)[:-1].encode())))
    no.append(("id_65_digits", _rep(ONE_BLOB, hid(1).encode(), hid(1).encode() + b"0")))
    no.append(("pack_id_63_digits", _rep(ONE_BLOB, hid(9).encode(), hid(9)[:-1].encode())))
    no.append(("id_not_hex", _rep(ONE_BLOB, hid(1).encode(), b"g" + hid(1)[1:].encode())))
    no.append(("id_not_a_string", _rep(ONE_BLOB, b'"' + hid(1).encode() + b'"', b"12")))
    no.append(("leading_zero", ONE(blob(1)).replace(b'"length":100', b'"length":0100')))
    no.append(("double_zero", ONE(blob(1)).replace(b'"offset":0', b'"offset":00')))
    no.append(("negative", ONE(blob(1)).replace(b'"offset":0', b'"offset":-1')))
    no.append(("fraction", ONE(blob(1)).replace(b'"length":100', b'"length":1.0')))
    no.append(("exponent", ONE(blob(1)).replace(b'"length":100', b'"length":1e3')))
    no.append(("plus_sign", ONE(blob(1)).replace(b'"length":100', b'"length":+1')))
    no.append(("two_pow_32", ONE(blob(1)).replace(b'"length":100', b'"length":4294967296')))
    no.append(("twenty_digits", ONE(blob(1)).replace(b'"length":100', b'"length":' + b"9" * 20)))
    no.append(("size_two_pow_32", compact({"packs": [dict(P1, size=4294967296)]})))
    no.append(("ulen_zero", ONE(blob(1, ulen=0))))
    no.append(("integer_as_string", ONE(blob(1)).replace(b'"length":100', b'"length":"100"')))
    no.append(("unknown_key_blob", ONE(dict(blob(1), extra=1))))
    no.append(("unknown_key_pack", ONE(blob(1), extra=None)))
    no.append(("unknown_key_root", compact({"packs": [P1], "extra": []})))
    no.append(("key_with_space", ONE_BLOB.replace(b'"offset"', b'"offset "')))
    no.append(("key_prefix", ONE_BLOB.replace(b'"offset"', b'"off"')))
    no.append(("duplicate_key_blob", ONE_BLOB.replace(b'"offset":0', b'"offset":0,"offset":0')))
    no.append(("duplicate_key_pack", ONE_BLOB.replace(b'"blobs":[', b'"blobs":[],"blobs":[')))
    no.append(("duplicate_key_root", b'{"packs":[],"packs":[]}'))
    for k in ("id", "type", "offset", "length"):
        o = blob(1)
        del o[k]
        no.append((f"blob_without_{k}", ONE(o)))
    no.append(("pack_without_id", compact({"packs": [{"blobs": [blob(1)]}]})))
    no.append(("pack_without_blobs", compact({"packs": [{"id": hid(9)}]})))
    no.append(("root_without_packs", compact({"packs_to_delete": [P1]})))
    no.append(("root_empty_object", b"{}"))
    no.append(("type_unknown", ONE(blob(1, "snapshot"))))
    no.append(("true_as_value", ONE(blob(1)).replace(b'"uncompressed_length":null', b'"uncompressed_length":true')))
    no.append(("packs_null", b'{"packs":null}'))
    no.append(("time_is_number", compact({"packs": [dict(P1, time=5)]})))
    no.append(("time_control_byte", compact({"packs": [dict(P1, time="ab")]}).replace(b'"ab"', b'"a\x01b"')))
    no.append(("time_high_byte", compact({"packs": [dict(P1, time="ab")]}).replace(b'"ab"', b'"a\xc3\xa9b"')))
    no.append(("nested_object_as_value", ONE(blob(1)).replace(b'"offset":0', b'"offset":{"a":0}')))
    no.append(("nested_array_as_value", ONE(blob(1)).replace(b'"offset":0', b'"offset":[0]')))
    no.append(("blob_is_array", ONE([1])))
    no.append(("pack_is_number", b'{"packs":[1]}'))
    no.append(("supersedes_number", compact({"supersedes": [1], "packs": []})))
    no.append(("supersedes_short_id", compact({"supersedes": [hid(1)[:-2]], "packs": []})))
    no.append(("supersedes_holds_object", compact({"supersedes": [{"id": hid(1), "blobs": []}], "packs": []})))
    no.append(("root_is_array", b"[" + compact(REF) + b"]"))
    no.append(("trailing_garbage", compact(REF) + b"x"))
    no.append(("trailing_object", compact(REF) + b"{}"))
    no.append(("trailing_comma_blobs", _rep(ONE_BLOB, b"}]}]}", b"},]}]}")))
    no.append(("trailing_comma_members", ONE_BLOB.replace(b'"uncompressed_length":null}', b'"uncompressed_length":null,}')))
    no.append(("missing_comma_blobs", compact(REF).replace(b"},{", b"}{", 1)))
    no.append(("missing_colon", ONE_BLOB.replace(b'"offset":0', b'"offset" 0')))
    no.append(("form_feed_as_whitespace", _rep(compact(REF), b"[", b"[\x0c")))
    no.append(("nul_as_whitespace", _rep(compact(REF), b",", b",\x00")))
    no.append(("leading_bom", b"\xef\xbb\xbf" + compact(REF)))
    no.append(("truncated_in_blob", compact(REF)[:200]))
    no.append(("truncated_last_byte", compact(REF)[:-1]))
    no.append(("truncated_in_id", compact(REF)[:40]))
    no.append(("empty_file", b""))
    no.append(("only_whitespace", b" \n"))
    no.append(("only_open_brace", b"{"))
    no.append(("unterminated_string", _rep(compact(REF), b'","blobs"', b',"blobs"')))
    no.append(("unterminated_time", compact({"packs": [dict(P1, time="x")]})[:-4]))
    no.append(("extra_closing_brackets", compact(REF) + b"]}"))
    no.append(("brackets_unbalanced", _rep(ONE_BLOB, b"}]}]}", b"}]]}")))
    return [(n, d, True) for n, d in yes] + [(n, d, False) for n, d in no]


CASES = _cases()
assert len({n for n, _, _ in CASES}) == len(CASES)


def random_index(rng: random.Random, n_packs: int, max_blobs: int, id_pool=None):
    """An index.IndexFile with random packs; ``id_pool``: draw blob ids from
    this list (so ids repeat) instead of making fresh ones."""
    from rustic_core_amd.index import IndexBlob, IndexFile, IndexPack
    f = IndexFile()
    for _ in range(n_packs):
        nb = rng.choice((0, 1, 2, rng.randrange(max_blobs + 1)))
        tpe = rng.randrange(2)
        p = IndexPack(rng.randbytes(32),
                      time=rng.choice((None, "2024-01-02T03:04:05.5+00:00")),
                      size=rng.choice((None, None, rng.randrange(1 << 32))))
        off = 0
        for _ in range(nb):
            ln = rng.choice((0, 1, rng.randrange(1 << 20), (1 << 32) - 1))
            bid = rng.choice(id_pool) if id_pool and rng.random() < 0.3 else rng.randbytes(32)
            t = tpe if rng.random() < 0.9 else 1 - tpe
            p.add(bid, t, off & 0xFFFFFFFF, ln, rng.choice((None, 1, rng.randrange(1, 1 << 32))))
            off += ln
        f.add(p, delete=rng.random() < 0.1)
    if rng.random() < 0.3:
        f.supersedes = [rng.randbytes(32) for _ in range(rng.randrange(3))]
    return f


def random_text(f, rng: random.Random) -> bytes:
    """``f`` as text in G: compact as to_json writes it, or with random
    whitespace and key order."""
    if rng.random() < 0.4:
        return f.to_json()
    return spaced(permuted(f.to_obj(), rng), rng)
