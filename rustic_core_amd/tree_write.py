"""Trees and snapshot files written on the host: a node with everything the
reference keeps of it, the serialiser of ``Tree::serialize`` and the one of a
saved ``SnapshotFile``.

Reference: ``backend/node.rs:78-291`` (``Node``, ``NodeType``, ``Metadata``,
``ExtendedAttribute``), ``blob/tree.rs:66-120`` (``Tree``, ``serialize``:
``serde_json::to_vec`` and a newline, the id is the SHA-256 of that),
``repofile/snapshotfile.rs:330-402`` (``SnapshotFile``).

A tree is read by ``tree.parse_tree_host``'s rule (keys ``Node`` does not know
are dropped, as serde drops them) and written in the declaration order of the
structs with their skip rules, whatever order the source text had.  Number
tokens and the ``mtime`` / ``atime`` / ``ctime`` strings go out exactly as they
came in: what the reference's ``RusticTime`` does to a time it has read is not
reproduced here.
"""
from __future__ import annotations

import hashlib
import json
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

from .errors import ErrorKind, RusticError
from .tree import NODE_TYPES, _check_node, _fail, _id, _pairs

EMPTY_TREE = b'{"nodes":[]}\n'
EMPTY_TREE_ID = hashlib.sha256(EMPTY_TREE).digest()

_OPTIONAL = ("mode", "mtime", "atime", "ctime", "uid", "gid", "user", "group")  # skip when none
_U64 = ("inode", "device_id", "size", "links")                                  # skip when 0


class _Int(int):
    """An integer token of a JSON text, kept as it was read."""
    tok: str

    def __new__(cls, tok: str):
        self = super().__new__(cls, tok)
        self.tok = tok
        return self


class _Float(float):
    """A number token with a fraction or an exponent, kept as it was read."""
    tok: str

    def __new__(cls, tok: str):
        self = super().__new__(cls, tok)
        self.tok = tok
        return self


def loads(text: bytes):
    """``json.loads`` that keeps number tokens and refuses a repeated key and
    a string that is no UTF-8 (a lone surrogate escape), as serde does."""
    s = bytes(text).decode("utf-8")
    out = json.loads(s, object_pairs_hook=_pairs, parse_int=_Int, parse_float=_Float)
    if "\\u" in s:
        json.dumps(out, ensure_ascii=False).encode("utf-8")  # raises for a lone surrogate
    return out


def quote(s: str) -> str:
    """A string as serde_json writes it: ``\\"``, ``\\\\``, the five letter
    escapes, ``\\u00xx`` for the other control characters, everything else as
    it is."""
    return json.dumps(s, ensure_ascii=False)


def _num(x) -> str:
    return getattr(x, "tok", None) or str(int(x))


def dump(v) -> str:
    """A JSON value as it was read by ``loads``: members in the text's order,
    number tokens unchanged, no spaces."""
    if v is None:
        return "null"
    if v is True or v is False:
        return "true" if v else "false"
    if isinstance(v, str):
        return quote(v)
    if isinstance(v, (_Int, _Float)):
        return v.tok
    if isinstance(v, int):
        return str(v)
    if isinstance(v, float):
        return repr(v)
    if isinstance(v, dict):
        return "{" + ",".join(quote(k) + ":" + dump(x) for k, x in v.items()) + "}"
    return "[" + ",".join(dump(x) for x in v) + "]"


@dataclass
class FullNode:
    """``Node`` with its flattened ``NodeType`` and ``Metadata``.  Ids are
    bytes; ``linktarget_raw`` and an extended attribute's value stay the
    base64 strings they were read as; ``device`` is set for dev and chardev
    only."""
    name: str
    type: str
    linktarget: Optional[str] = None
    linktarget_raw: Optional[str] = None
    device: Optional[int] = None
    mode: Optional[int] = None
    mtime: Optional[str] = None
    atime: Optional[str] = None
    ctime: Optional[str] = None
    uid: Optional[int] = None
    gid: Optional[int] = None
    user: Optional[str] = None
    group: Optional[str] = None
    inode: int = 0
    device_id: int = 0
    size: int = 0
    links: int = 0
    extended_attributes: List[Tuple[str, Optional[str]]] = field(default_factory=list)
    content: Optional[List[bytes]] = None
    subtree: Optional[bytes] = None


def node_from_json(n: dict) -> FullNode:
    """A node object (as ``loads`` gives it) by ``Node``'s deserialiser."""
    _check_node(n)
    tpe = n["type"]
    out = FullNode(n["name"], tpe)
    if tpe == "symlink":
        out.linktarget, out.linktarget_raw = n["linktarget"], n.get("linktarget_raw")
    elif tpe in ("dev", "chardev"):
        out.device = n.get("device", 0)
    for k in _OPTIONAL:
        setattr(out, k, n.get(k))
    for k in _U64:
        setattr(out, k, n.get(k, 0))
    out.extended_attributes = [(x["name"], x.get("value")) for x in n.get("extended_attributes", [])]
    content = n.get("content")
    out.content = None if content is None else [_id(i) for i in content]
    out.subtree = None if n.get("subtree") is None else _id(n["subtree"])
    return out


def parse_tree_full(text: bytes) -> List[FullNode]:
    """The nodes of one tree blob with everything ``Node`` holds.  What does
    not parse raises as ``tree.parse_tree_host`` does; a dir node without a
    subtree is a node like any other."""
    try:
        root = loads(text)
        if not isinstance(root, dict) or "nodes" not in root:
            raise ValueError("missing field `nodes`")
        nodes = root["nodes"] if root["nodes"] is not None else []
        if not isinstance(nodes, list):
            raise ValueError("nodes is no sequence")
        return [node_from_json(n) for n in nodes]
    except (ValueError, TypeError, RecursionError) as e:
        raise _fail(str(e)) from e


def serialize_node(n: FullNode) -> str:
    if n.type not in NODE_TYPES:
        raise RusticError(ErrorKind.InvalidInput, f"unknown node type `{n.type}`")
    p = ['"name":' + quote(n.name), '"type":' + quote(n.type)]
    if n.type == "symlink":
        p.append('"linktarget":' + quote(n.linktarget or ""))
        if n.linktarget_raw is not None:
            p.append('"linktarget_raw":' + quote(n.linktarget_raw))
    elif n.type in ("dev", "chardev"):
        p.append('"device":' + _num(n.device or 0))
    for k in _OPTIONAL:
        v = getattr(n, k)
        if v is not None:
            p.append(f'"{k}":' + (quote(v) if isinstance(v, str) else _num(v)))
    for k in _U64:
        v = getattr(n, k)
        if int(v) != 0:
            p.append(f'"{k}":' + _num(v))
    if n.extended_attributes:
        p.append('"extended_attributes":[' + ",".join(
            '{"name":' + quote(a) + ',"value":' + ("null" if v is None else quote(v)) + "}"
            for a, v in n.extended_attributes) + "]")
    p.append('"content":' + ("null" if n.content is None else
                             "[" + ",".join('"' + bytes(i).hex() + '"' for i in n.content) + "]"))
    if n.subtree is not None:
        p.append('"subtree":"' + bytes(n.subtree).hex() + '"')
    return "{" + ",".join(p) + "}"


def serialize_tree(nodes: Sequence[FullNode]) -> Tuple[bytes, bytes]:
    """``Tree::serialize``: (text, id)."""
    text = ('{"nodes":[' + ",".join(serialize_node(n) for n in nodes) + "]}\n").encode("utf-8")
    return text, hashlib.sha256(text).digest()


# ---- snapshot files -------------------------------------------------------------

def parse_snapshot(text: bytes) -> dict:
    """A snapshot file's object, members and number tokens as read."""
    try:
        o = loads(text)
        if not isinstance(o, dict):
            raise ValueError("a snapshot is a map")
        for k in ("time", "tree", "paths"):
            if k not in o:
                raise ValueError(f"missing field `{k}`")
        _id(o["tree"])
        return o
    except (ValueError, TypeError, RecursionError) as e:
        raise RusticError(ErrorKind.Internal,
                          f"Failed to deserialize snapshot from JSON. ({e})") from e


def _string_list(v) -> str:
    return "[" + ",".join(quote(s) for s in sorted(set(v or []))) + "]"  # a BTreeSet


def serialize_snapshot(o: dict, snap_id: Optional[bytes]) -> bytes:
    """``serde_json::to_vec(&SnapshotFile)``: the struct's order and skip
    rules; ``snap_id`` is the struct's ``id`` (the id the file was loaded
    under: written unless it is none or all zero, as ``save_file`` does with a
    snapshot that came from the repository)."""
    p = ['"time":' + dump(o["time"])]
    if o.get("program_version"):
        p.append('"program_version":' + quote(o["program_version"]))
    if o.get("parent") is not None:
        p.append('"parent":' + quote(o["parent"]))
    if o.get("parents"):
        p.append('"parents":' + dump(o["parents"]))
    p.append('"tree":' + quote(o["tree"]))
    if o.get("label"):
        p.append('"label":' + quote(o["label"]))
    p.append('"paths":' + _string_list(o["paths"]))
    p.append('"hostname":' + quote(o.get("hostname") or ""))
    p.append('"username":' + quote(o.get("username") or ""))
    p.append('"uid":' + _num(o.get("uid") or 0))
    p.append('"gid":' + _num(o.get("gid") or 0))
    p.append('"tags":' + _string_list(o.get("tags")))
    if o.get("original") is not None:
        p.append('"original":' + quote(o["original"]))
    if o.get("delete") not in (None, "NotSet"):
        p.append('"delete":' + dump(o["delete"]))
    for k in ("summary", "description"):
        if o.get(k) is not None:
            p.append(f'"{k}":' + dump(o[k]))
    if snap_id is not None and any(bytes(snap_id)):
        p.append('"id":"' + bytes(snap_id).hex() + '"')
    return ("{" + ",".join(p) + "}").encode("utf-8")
