"""Hand-built tree blobs for the grammar G_T of rcdc_tree_parse: (name, bytes,
in G_T?).  The accepted ones cover the forms tree blobs come in; the rejected
ones break one rule of G_T each.  Also the generator of random trees."""
import json
import random

from tests.index_json_cases import hid, permuted

TIME = "2024-05-06T07:08:09.123456789+02:00"
TYPES = ("file", "dir", "symlink", "dev", "chardev", "fifo", "socket")


def compact(o) -> bytes:
    """serde_json::to_vec: compact, strings as they are (no \\u for non-ASCII)."""
    return json.dumps(o, separators=(",", ":"), ensure_ascii=False).encode()


def serialize(o) -> bytes:
    """Tree::serialize (blob/tree.rs:110-120): the compact text and a newline."""
    return compact(o) + b"\n"


def spaced(o, rng) -> bytes:
    """JSON text with random runs of the four whitespace bytes between any
    two tokens and around the root."""
    ws = lambda: "".join(rng.choice(" \t\n\r") for _ in range(rng.choice((0, 0, 1, 2, 5))))
    s = lambda x: json.dumps(x, ensure_ascii=False)

    def emit(x):
        if isinstance(x, dict):
            return "{" + ws() + ",".join(ws() + s(k) + ws() + ":" + ws() + emit(v) + ws()
                                         for k, v in x.items()) + "}"
        if isinstance(x, list):
            return "[" + ws() + ",".join(ws() + emit(v) + ws() for v in x) + "]"
        return s(x)
    return (ws() + emit(o) + ws()).encode()


def meta(n: int) -> dict:
    """Metadata as rustic writes it (backend/node.rs:245-276; zero u64 fields
    and None are skipped)."""
    return {"mode": 33188, "mtime": TIME, "atime": TIME, "ctime": TIME, "uid": 1000, "gid": 100,
            "user": "alice", "group": "users", "inode": 1000 + n, "device_id": 64769,
            "size": 4096 * n, "links": 1}


def file_node(name, ids, **kw) -> dict:
    """Node's field order: name, type, metadata, content, subtree."""
    return dict({"name": name, "type": "file"}, **kw, content=[hid(i) for i in ids])


def dir_node(name, tree, **kw) -> dict:
    return dict({"name": name, "type": "dir"}, **kw, content=None, subtree=hid(tree))


def other_node(name, tpe, **kw) -> dict:
    o = {"name": name, "type": tpe}
    if tpe == "symlink":
        o["linktarget"] = "../target"
    if tpe in ("dev", "chardev"):
        o["device"] = 2049
    return dict(o, **kw, content=None)


def tree(*nodes) -> dict:
    return {"nodes": list(nodes)}


RUSTIC = tree(file_node("a.txt", [1, 2, 3], **meta(1)), dir_node("sub", 40, **meta(2)),
              file_node("empty", [], **meta(3)), other_node("link", "symlink", **meta(4)))
ONE_FILE = serialize(tree(file_node("f", [1, 2])))
ONE_DIR = serialize(tree(dir_node("d", 9)))


def _rep(src: bytes, old: bytes, new: bytes) -> bytes:
    assert src.count(old) >= 1, (src, old)
    return src.replace(old, new, 1)


def _named(raw: bytes) -> bytes:
    """ONE_FILE with the raw bytes ``raw`` between the quotes of its name."""
    return _rep(ONE_FILE, b'"name":"f"', b'"name":"' + raw + b'"')


def _cases():
    rng = random.Random(11)
    yes, no = [], []
    yes.append(("rustic_style", serialize(RUSTIC)))
    # restic: Go's encoding/json writes <, > and & as \u003c, \u003e, \u0026,
    # keeps "content":null for a dir and puts "subtree" before it
    yes.append(("restic_style", _rep(_rep(serialize(tree(
        dict({"name": "NAME", "type": "file"}, **meta(1), content=[hid(5), hid(6)]),
        dict({"name": "d", "type": "dir"}, **meta(2), subtree=hid(41), content=None))),
        b"NAME", b"a\\u003cb\\u003e\\u0026c"), b'"user":"alice"', b'"user":"al\\u0026ice"')))
    yes.append(("every_node_type", serialize(tree(
        file_node("f", [1]), dir_node("d", 2), *[other_node(t, t) for t in TYPES[2:]]))))
    yes.append(("content_null", serialize(tree(dict({"name": "f", "type": "file"}, content=None)))))
    yes.append(("content_absent", serialize(tree({"name": "f", "type": "file"}))))
    yes.append(("content_empty", serialize(tree(file_node("f", [])))))
    yes.append(("non_dir_with_subtree", serialize(tree(
        dict(file_node("f", [1, 2]), subtree=hid(7)), dict(other_node("l", "symlink"), subtree=hid(8)),
        dir_node("d", 9)))))
    yes.append(("non_file_with_content", serialize(tree(
        dict(dir_node("d", 9), content=[hid(1), hid(2)]),
        dict(other_node("s", "socket"), content=[hid(3)]), file_node("f", [4])))))
    yes.append(("subtree_null", serialize(tree(dict(file_node("f", [1]), subtree=None)))))
    yes.append(("nodes_null", b'{"nodes":null}\n'))
    yes.append(("nodes_empty", b'{"nodes":[]}\n'))
    yes.append(("no_trailing_newline", compact(RUSTIC)))
    for i in range(3):
        yes.append((f"keys_permuted_{i}", compact(permuted(RUSTIC, rng))))
    yes.append(("every_whitespace", spaced(RUSTIC, rng)))
    yes.append(("pretty", json.dumps(RUSTIC, indent=2).encode()))
    yes.append(("whitespace_around_root", b" \t\r\n" + compact(RUSTIC) + b"\n \t\r"))
    yes.append(("name_escaped_quote", _named(b'a\\"b')))
    yes.append(("name_escaped_backslash", _named(b"a\\\\")))
    yes.append(("name_backslash_then_quote", _named(b'a\\\\\\"')))
    yes.append(("name_every_escape", _named(b'\\"\\\\\\/\\b\\f\\n\\r\\t\\u0000\\uFFFF\\ud7ff\\ue000')))
    yes.append(("name_unicode_escape", _named(b"caf\\u00e9")))
    yes.append(("name_utf8_2_3_4_bytes", _named("é€\U0001F600߿ࠀ￿\U0010FFFF".encode())))
    yes.append(("name_is_content_user_is_subtree", serialize(tree(
        dict(file_node("content", [1]), user="subtree", group='"content":["x"]')))))
    yes.append(("name_of_brackets", serialize(tree(file_node("]}[{,:", [1]), dir_node("[[[[", 2)))))
    yes.append(("xattr_named_content", serialize(tree(dict(
        {"name": "f", "type": "file"}, extended_attributes=[
            {"name": "content", "value": "YWJj"}, {"name": "user.x", "value": None},
            {"value": "", "name": "subtree"}, {"name": "only"}], content=[hid(1), hid(2)])))))
    yes.append(("xattrs_empty_after_content", serialize(tree(
        dict(file_node("f", [1]), extended_attributes=[]), file_node("g", [2, 3])))))
    yes.append(("null_metadata", serialize(tree(dict(
        {"name": "f", "type": "file"}, mode=None, uid=None, gid=None, mtime=None, atime=None,
        ctime=None, user=None, group=None), dict(other_node("l", "symlink"), linktarget_raw=None)))))
    yes.append(("integer_limits", serialize(tree(dict(
        {"name": "f", "type": "file"}, mode=4294967295, uid=0, inode=18446744073709551615,
        size=0, links=18446744073709551615, device=1)))))
    yes.append(("upper_case_hex", serialize(tree(file_node("f", [1, 2]))).replace(
        hid(1).encode(), hid(1).upper().encode())))
    yes.append(("linktarget_raw_text", serialize(tree(dict(
        other_node("l", "symlink"), linktarget_raw="L3RtcC9h")))))

    no.append(("duplicate_content", _rep(ONE_FILE, b'"content":[', b'"content":[],"content":[')))
    no.append(("duplicate_name", _rep(ONE_FILE, b'"name":"f"', b'"name":"f","name":"f"')))
    no.append(("unknown_key", serialize(tree(dict(file_node("f", [1]), generic_attributes={})))))
    no.append(("unknown_key_null", serialize(tree(dict(file_node("f", [1]), extra=None)))))
    no.append(("escaped_key", _rep(ONE_FILE, b'"name":', b'"n\\u0061me":')))
    no.append(("escaped_key_content", _rep(ONE_FILE, b'"content":', b'"c\\u006fntent":')))
    no.append(("id_63_digits", _rep(ONE_FILE, hid(1).encode(), hid(1)[:-1].encode())))
    no.append(("id_65_digits", _rep(ONE_FILE, hid(1).encode(), hid(1).encode() + b"0")))
    no.append(("second_id_63_digits", _rep(ONE_FILE, hid(2).encode(), hid(2)[:-1].encode())))
    no.append(("subtree_63_digits", _rep(ONE_DIR, hid(9).encode(), hid(9)[:-1].encode())))
    no.append(("id_not_hex", _rep(ONE_FILE, hid(1).encode(), b"g" + hid(1)[1:].encode())))
    no.append(("subtree_not_hex", _rep(ONE_DIR, hid(9).encode(), b"x" + hid(9)[1:].encode())))
    no.append(("id_with_escape", _rep(ONE_FILE, hid(1).encode(), b"\\u0030" + hid(1)[1:].encode())))
    no.append(("id_with_escape_64_bytes", _rep(ONE_FILE, hid(1).encode(),
                                               b"\\u0030" + hid(1)[6:].encode())))
    no.append(("id_is_number", _rep(ONE_FILE, b'"' + hid(1).encode() + b'"', b"12")))
    no.append(("id_is_null", _rep(ONE_FILE, b'"' + hid(2).encode() + b'"', b"null")))
    no.append(("unknown_type", _rep(ONE_FILE, b'"type":"file"', b'"type":"door"')))
    no.append(("type_upper_case", _rep(ONE_FILE, b'"type":"file"', b'"type":"File"')))
    no.append(("type_with_escape", _rep(ONE_FILE, b'"type":"file"', b'"type":"f\\u0069le"')))
    no.append(("type_absent", serialize(tree({"name": "f", "content": []}))))
    no.append(("name_absent", serialize(tree({"type": "file", "content": []}))))
    no.append(("name_null", _rep(ONE_FILE, b'"name":"f"', b'"name":null')))
    no.append(("symlink_without_linktarget", serialize(tree({"name": "l", "type": "symlink"}))))
    no.append(("linktarget_null", serialize(tree({"name": "l", "type": "symlink", "linktarget": None}))))
    no.append(("dir_without_subtree", serialize(tree({"name": "d", "type": "dir"}))))
    no.append(("dir_subtree_null", serialize(tree({"name": "d", "type": "dir", "subtree": None}))))
    no.append(("mode_two_pow_32", serialize(tree(dict(file_node("f", [1]), mode=4294967296)))))
    no.append(("size_two_pow_64", serialize(tree(dict(file_node("f", [1]), size=18446744073709551616)))))
    no.append(("size_null", serialize(tree(dict(file_node("f", [1]), size=None)))))
    no.append(("leading_zero", _rep(serialize(tree(dict(file_node("f", [1]), size=7))),
                                    b'"size":7', b'"size":07')))
    no.append(("negative_number", serialize(tree(dict(file_node("f", [1]), uid=-1)))))
    no.append(("fraction", _rep(serialize(tree(dict(file_node("f", [1]), size=7))),
                                b'"size":7', b'"size":7.0')))
    no.append(("exponent", _rep(serialize(tree(dict(file_node("f", [1]), size=7))),
                                b'"size":7', b'"size":7e0')))
    no.append(("number_as_string", serialize(tree(dict(file_node("f", [1]), size="7")))))
    no.append(("raw_control_byte_in_name", _named(b"a\x01b")))
    no.append(("raw_newline_in_name", _named(b"a\nb")))
    no.append(("raw_del_is_fine_but_tab_is_not", _named(b"a\x7f\tb")))
    no.append(("bad_escape", _named(b"a\\xb")))
    no.append(("bad_escape_u_3_digits", _named(b"a\\u12g4")))
    no.append(("escape_ud800", _named(b"\\ud800")))
    no.append(("escape_surrogate_pair", _named(b"\\ud83d\\ude00")))
    no.append(("escape_udfff", _named(b"\\uDFFF")))
    no.append(("utf8_overlong_2", _named(b"\xc0\xaf")))
    no.append(("utf8_overlong_3", _named(b"\xe0\x9f\xbf")))
    no.append(("utf8_overlong_4", _named(b"\xf0\x8f\xbf\xbf")))
    no.append(("utf8_truncated", _named(b"\xe2\x82")))
    no.append(("utf8_truncated_4", _named(b"\xf0\x9f\x98")))
    no.append(("utf8_lone_continuation", _named(b"\x80")))
    no.append(("utf8_surrogate", _named(b"\xed\xa0\x80")))
    no.append(("utf8_above_10ffff", _named(b"\xf4\x90\x80\x80")))
    no.append(("utf8_f5", _named(b"\xf5\x80\x80\x80")))
    no.append(("utf8_bad_in_user", serialize(tree(dict(file_node("f", [1]), user="U"))).replace(b'"U"', b'"\xff"')))
    no.append(("unclosed_string", _rep(ONE_FILE, b'"name":"f"', b'"name":"f')))
    no.append(("unclosed_last_string", ONE_FILE[:ONE_FILE.rindex(b'"')]))
    no.append(("string_ends_in_backslash", _named(b"a\\")))
    no.append(("depth_6", serialize(tree(dict({"name": "f", "type": "file"}, extended_attributes=[
        {"name": "a", "value": ["x"]}])))))
    no.append(("depth_6_object", serialize(tree(dict({"name": "f", "type": "file"}, extended_attributes=[
        {"name": "a", "value": {"x": 1}}])))))
    no.append(("content_of_arrays", _rep(ONE_FILE, b'"content":[', b'"content":[[],')))
    no.append(("xattrs_null", serialize(tree(dict(file_node("f", [1]), extended_attributes=None)))))
    no.append(("xattr_is_string", serialize(tree(dict({"name": "f", "type": "file"},
                                                      extended_attributes=[hid(1)])))))
    no.append(("xattr_without_name", serialize(tree(dict({"name": "f", "type": "file"},
                                                         extended_attributes=[{"value": "eA=="}])))))
    no.append(("xattr_unknown_key", serialize(tree(dict({"name": "f", "type": "file"}, extended_attributes=[
        {"name": "a", "value": None, "x": 1}])))))
    no.append(("xattr_duplicate_name", _rep(serialize(tree(dict(
        {"name": "f", "type": "file"}, extended_attributes=[{"name": "a"}]))),
        b'{"name":"a"}', b'{"name":"a","name":"a"}')))
    no.append(("second_root_key", _rep(ONE_FILE, b"]}\n", b'],"x":1}\n')))
    no.append(("second_nodes_key", _rep(ONE_FILE, b"]}\n", b'],"nodes":[]}\n')))
    no.append(("other_root_key", b'{"tree":[]}\n'))
    no.append(("root_empty_object", b"{}\n"))
    no.append(("root_is_array", b"[" + compact(RUSTIC) + b"]"))
    no.append(("nodes_is_object", b'{"nodes":{}}\n'))
    no.append(("node_is_array", b'{"nodes":[[]]}\n'))
    no.append(("node_is_number", b'{"nodes":[1]}\n'))
    no.append(("node_is_empty_object", b'{"nodes":[{}]}\n'))
    no.append(("trailing_non_whitespace", serialize(RUSTIC) + b"x"))
    no.append(("trailing_object", serialize(RUSTIC) + b"{}"))
    no.append(("trailing_comma_content", _rep(ONE_FILE, b'"]', b'",]')))
    no.append(("trailing_comma_nodes", _rep(ONE_FILE, b"}]}", b"},]}")))
    no.append(("trailing_comma_members", _rep(ONE_FILE, b"]}]}", b"],}]}")))
    no.append(("missing_comma_content", _rep(ONE_FILE, hid(1).encode() + b'","', hid(1).encode() + b'""')))
    no.append(("missing_comma_nodes", _rep(serialize(tree(file_node("f", [1]), file_node("g", [2]))),
                                           b"},{", b"}{")))
    no.append(("missing_colon", _rep(ONE_FILE, b'"name":', b'"name" ')))
    no.append(("backslash_outside_string", _rep(ONE_FILE, b',"type"', b',\\"type"')))
    no.append(("form_feed_as_whitespace", _rep(ONE_FILE, b"[", b"[\x0c")))
    no.append(("leading_bom", b"\xef\xbb\xbf" + ONE_FILE))
    no.append(("truncated_in_id", ONE_FILE[:60]))
    no.append(("truncated_last_byte", ONE_FILE[:-2]))
    no.append(("empty_blob", b""))
    no.append(("only_whitespace", b" \n"))
    no.append(("only_open_brace", b"{"))
    no.append(("brackets_unbalanced", _rep(ONE_FILE, b"]}]}", b"]]}")))
    no.append(("extra_closing_brackets", ONE_FILE[:-1] + b"]}\n"))
    no.append(("true_as_value", _rep(ONE_FILE, b'"name":"f"', b'"name":true')))
    return [(n, d, True) for n, d in yes] + [(n, d, False) for n, d in no]


CASES = _cases()
assert len({n for n, _, _ in CASES}) == len(CASES)

_NAMES = ("a", "file.txt", "café", "€\U0001F600", 'q"uote', "back\\slash", "tab\there",
          "content", "subtree", "]}[{", "x" * 70, "\\\\\"", "")


def random_tree(rng: random.Random, max_nodes: int = 12, max_ids: int = 6) -> dict:
    """A tree object in G_T with random nodes; ids are random."""
    rid = lambda: rng.randbytes(32).hex()
    nodes = []
    for k in range(rng.choice((0, 1, 2, rng.randrange(max_nodes + 1)))):
        tpe = rng.choice(TYPES + ("file", "file", "dir"))
        n = {"name": rng.choice(_NAMES), "type": tpe}
        if rng.random() < 0.7:
            n.update(meta(k))
        if rng.random() < 0.2:
            n.update(mode=None, user=None, mtime=None)
        if tpe == "symlink":
            n["linktarget"] = rng.choice(_NAMES)
        if tpe in ("dev", "chardev") and rng.random() < 0.7:
            n["device"] = rng.randrange(1 << 64)
        if rng.random() < 0.2:
            n["extended_attributes"] = [dict(name=rng.choice(_NAMES), value=rng.choice((None, "YQ==")))
                                        for _ in range(rng.randrange(3))]
        r = rng.random()
        if tpe == "file" or r < 0.15:
            n["content"] = [rid() for _ in range(rng.choice((0, 1, 2, rng.randrange(max_ids + 1))))]
        elif r < 0.6:
            n["content"] = None
        if tpe == "dir" or rng.random() < 0.1:
            n["subtree"] = rid()
        elif rng.random() < 0.1:
            n["subtree"] = None
        nodes.append(n)
    return {"nodes": nodes if nodes or rng.random() < 0.8 else None}


def random_text(o, rng: random.Random) -> bytes:
    """``o`` as text in G_T: as Tree::serialize writes it, or with random
    whitespace and key order."""
    if rng.random() < 0.5:
        return serialize(o)
    return spaced(permuted(o, rng), rng)


def flipped(text: bytes, rng: random.Random) -> bytes:
    """``text`` with one bit of one byte flipped."""
    b = bytearray(text)
    b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
    return bytes(b)
