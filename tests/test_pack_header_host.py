"""CPU: the model of the pack header parser (tests/pack_header_model.py)
against ``pack.parse_header`` / ``pack.header_size``; the parser's bound and
tile through ctypes; ``headers.PackChecker``; and ``headers.read_headers`` /
``headers.repair_index`` with ``device=None`` -- the host rule the device
path is held against -- over a repository built in memory, with every error
branch of PackHeader::from_file."""
import hashlib
import warnings

import numpy as np
import pytest

from tests import pack_header_model as model
from tests.pack_header_cases import TABLE, bid, random_header, run
from tests.pack_header_model import BAD_TYPE, CUT_SHORT, OK


# ---- the model ---------------------------------------------------------------------------

def _against_parse_header(header: bytes):
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.pack import header_size, parse_header
    j = model.judge(header)
    if j.status in (BAD_TYPE, CUT_SHORT):
        with pytest.raises(RusticError) as e:
            parse_header(header)
        assert e.value.kind == ErrorKind.Internal
        assert f"at byte {j.err_pos}" in str(e.value)
        assert ("cut short" in str(e.value)) == (j.status == CUT_SHORT)
        return j
    got = parse_header(header)  # it knows no overflow: offsets are Python ints
    # header_size goes by the blobs, as PackHeaderRef::size does: a 41-byte entry whose
    # uncompressed length is 0 counts as 37 there
    pos = zero = 0
    for g in got:
        zero += header[pos] >= 2 and not g.uncompressed_len
        pos += 41 if header[pos] >= 2 else 37
    assert pos == len(header) and header_size(got) == len(header) - 4 * zero
    if j.status == OK:
        assert [(g.type, g.offset, g.length, g.uncompressed_len, g.id) for g in got] == j.entries
    else:
        assert got[-1].offset + got[-1].length > 0xFFFFFFFF
    return j


@pytest.mark.parametrize("name,header,status", TABLE, ids=[c[0] for c in TABLE])
def test_table(name, header, status):
    assert _against_parse_header(header).status == status


def test_random_headers():
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(300):
        seen.add(_against_parse_header(random_header(rng)).status)
    assert seen == {OK, BAD_TYPE, CUT_SHORT}


def test_collect():
    """Typing, numbering and the two sizes, on a batch written out by hand."""
    from rustic_core_amd.index import IndexPack
    hs = [run([0, 2]), run([1]), b"\x07", run([3, 0]), b"", run([2])]
    c = model.collect(hs, (5, 9))
    assert c.status == [OK, OK, BAD_TYPE, OK, OK, OK]
    assert [(r.type, r.number, r.first, r.count) for r in c.records] == \
        [(0, 5, 0, 2), (1, 9, 0, 1), (0, 0, 0, 0), (1, 10, 1, 2), (0, 6, 2, 0), (0, 7, 2, 1)]
    assert (c.records[3].data, c.records[3].tree) == (1, 1)  # mixed, filed under tree
    assert c.packs == [3, 2] and [len(i) for i in c.ids] == [3, 3]
    assert [l[0] for l in c.locs[1]] == [9, 10, 10]
    for h, r in zip(hs, c.records):
        if r.status == OK:
            p = IndexPack(b"\0" * 32)
            for t, off, length, ulen, id_ in model.judge(h).entries:
                p.add(id_, t, off, length, ulen or None)
            assert r.pack_size == p.pack_size() and r.size == 32 + len(h)


def test_pattern_against_the_model():
    """The arithmetic of ``pack_header_cases.Pattern`` (what the device test
    of more than 2^20 headers expects) against ``collect`` at 3 000 headers:
    every field of every record and both entry arrays in full."""
    from tests.pack_header_cases import Pattern
    p = Pattern(3000, (7, 1 << 20))
    hs = p.headers()
    assert len(hs) == 3000 and hs[:4] == [b"", hs[1], hs[2], hs[3]] and hs[999][0] == 4
    assert [len(h) for h in hs[:4]] == [0, 37, 37, 82] and len({h[5:9] for h in hs[1::4]}) == 750
    c = model.collect(hs, (7, 1 << 20))
    assert c.status.count(BAD_TYPE) == 3 and c.status.count(OK) == 2997
    for k in model.Record._fields:
        assert [getattr(r, k) for r in c.records] == p.records[k].tolist(), k
    assert c.packs == p.packs
    for t in (0, 1):
        assert b"".join(c.ids[t]) == p.ids[t].tobytes(), t
        assert [list(l) for l in c.locs[t]] == p.locs[t].tolist(), t


def test_bound_and_tile():
    from rustic_core_amd import _lib, headers
    L = _lib.lib()
    for n in (0, 1, 36, 37, 73, 74, 41 * 100, 2 ** 40 + 5):
        assert L.rcdc_pack_header_parse_bound(n) == n // 37 == headers.parse_bound(n)
    tile = L.rcdc_pack_header_parse_tile()
    assert tile == headers.parse_tile() and tile % 16 == 0 and tile >= 41
    assert -(-tile // 37) <= 64  # a tile's entries fit one wave


# ---- PackChecker ---------------------------------------------------------------------------

def _index_pack(name, n=3, tpe=0, size=None):
    from rustic_core_amd.index import IndexPack
    p = IndexPack(bid(f"pack:{name}"), size=size)
    for k in range(n):
        p.add(bid(f"{name}:{k}"), tpe, 50 * k, 50, 70 if k % 2 else None)
    return p


def test_pack_checker():
    from rustic_core_amd.headers import PackChecker
    from rustic_core_amd.index import IndexFile
    from rustic_core_amd.pack import header_size
    a, b, c, d, e = (_index_pack(n) for n in "abcde")
    listed = {a.id: a.pack_size(), b.id: b.pack_size() + 1, c.id: c.pack_size(),
              e.id: e.pack_size(), bid("pack:only listed"): 777}
    ck = PackChecker(listed)
    # a is fine; b's size differs; d is not listed; c sits in packs_to_delete and is fine
    new, changed = ck.check_pack(IndexFile([a, b, d], [c]))
    assert changed and new.packs == [a] and new.packs_to_delete == [c]
    assert ck.dropped == [d.id]
    assert ck.packs_to_read == [(b.id, header_size(b.blobs) + 32, b.pack_size() + 1)]
    # a again (indexed twice: dropped), e fine
    new, changed = ck.check_pack(IndexFile([a, e]))
    assert changed and new.packs == [e] and ck.dropped == [d.id, a.id]
    # nothing left to complain about
    new, changed = ck.check_pack(IndexFile([]))
    assert not changed and not new.packs
    assert ck.into_pack_to_read() == [(b.id, header_size(b.blobs) + 32, b.pack_size() + 1),
                                      (bid("pack:only listed"), None, 777)]
    # read_all: every listed pack is read again, with its header size as the hint
    ck = PackChecker({a.id: a.pack_size()})
    new, changed = ck.check_pack(IndexFile([a]), read_all=True)
    assert changed and not new.packs
    assert ck.into_pack_to_read() == [(a.id, 32 + 37 * 2 + 41, a.pack_size())]
    # an unchanged file stays as it is
    ck = PackChecker({a.id: a.pack_size()})
    new, changed = ck.check_pack(IndexFile([a]))
    assert not changed and new.packs == [a] and ck.into_pack_to_read() == []
    # "size" in the index file is what pack_size() answers
    f = _index_pack("f", size=4242)
    ck = PackChecker({f.id: 4242})
    assert not ck.check_pack(IndexFile([f]))[1]


# ---- a repository in memory -----------------------------------------------------------------

class HostKey:
    """nonce || data || tag with the sizes of the real sealing: all the host
    path needs of a key."""

    def seal(self, data: bytes, nonce=b"n" * 16) -> bytes:
        return nonce + data + hashlib.sha256(b"mac" + nonce + data).digest()[:16]

    def decrypt_data(self, data: bytes) -> bytes:
        from rustic_core_amd.errors import ErrorKind, RusticError
        from rustic_core_amd.read import MAC_MESSAGE, SHORT_MESSAGE
        if len(data) < 16:
            raise RusticError(ErrorKind.Cryptography, SHORT_MESSAGE)
        nonce, body, tag = data[:16], data[16:-16], data[-16:]
        if len(data) < 32 or hashlib.sha256(b"mac" + nonce + body).digest()[:16] != tag:
            raise RusticError(ErrorKind.Cryptography, MAC_MESSAGE)
        return body


def make_pack(key, types, name, header=None):
    """(pack bytes, IndexPack): blobs of 60 + 3k bytes, then the sealed
    header (``header``: these plain bytes in its place), then its length."""
    from rustic_core_amd.index import IndexPack
    lengths = [60 + 3 * k for k in range(len(types))]
    ids = [bid(f"{name}:{k}") for k in range(len(types))]
    ulens = [500 + k for k in range(len(types))]
    plain = run(types, lengths, ids, ulens)
    body = b"".join(hashlib.sha256(i).digest() * 4 for i in ids)
    blobs, off = b"", 0
    ip = IndexPack(b"")
    for t, n, i, u in zip(types, lengths, ids, ulens):
        blobs += body[:n]
        ip.add(i, t & 1, off, n, u if t >= 2 else None)
        off += n
    sealed = key.seal(plain if header is None else header)
    pack = blobs + sealed + len(sealed).to_bytes(4, "little")
    ip.id = hashlib.sha256(pack).digest()
    return pack, ip


class Repo:
    def __init__(self, packs):
        self.packs = dict(packs)
        self.calls = []

    def listed(self):
        return {i: len(p) for i, p in self.packs.items()}

    def read_partial(self, pack_id, offset, length):
        self.calls.append((bytes(pack_id), offset, length))
        assert 0 <= offset and offset + length <= len(self.packs[bytes(pack_id)])
        return self.packs[bytes(pack_id)][offset:offset + length]


def test_read_headers_host():
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.headers import (CONTENTS_MESSAGE, READ_MESSAGE, HeaderResult,
                                         read_headers)
    from rustic_core_amd.pack import header_size
    from rustic_core_amd.read import MAC_MESSAGE
    key = HostKey()
    good, gp = make_pack(key, [0, 2, 0, 2, 2], "good")
    tree, tp = make_pack(key, [3, 1, 3], "tree")
    mixed, mp = make_pack(key, [0, 1, 3], "mixed")
    empty, ep = make_pack(key, [], "empty")
    repo = Repo({p.id: f for f, p in ((good, gp), (tree, tp), (mixed, mp), (empty, ep))})
    hint = lambda p: header_size(p.blobs) + 32
    res = read_headers(key, [(gp.id, hint(gp), len(good)), (tp.id, None, len(tree)),
                             (mp.id, hint(mp) + 100, len(mixed)), (ep.id, 5, len(empty))],
                       repo.read_partial, device=None)
    assert all(isinstance(r, HeaderResult) for r in res)
    assert [r.index_pack.blobs for r in res] == [gp.blobs, tp.blobs, mp.blobs, []]
    assert [(r.type, r.count, r.data, r.tree, r.mixed, r.pack_size) for r in res] == \
        [(0, 5, 5, 0, False, len(good)), (1, 3, 0, 3, False, len(tree)),
         (0, 3, 1, 2, True, len(mixed)), (0, 0, 0, 0, False, len(empty))]
    # the reads: one with a right or a large guess, two where it was too small
    by = lambda i: [c[1:] for c in repo.calls if c[0] == i]
    assert by(gp.id) == [(len(good) - hint(gp) - 4, hint(gp) + 4)]
    assert by(tp.id) == [(len(tree) - 4, 4), (len(tree) - hint(tp) - 4, hint(tp))]
    assert by(mp.id) == [(len(mixed) - hint(mp) - 104, hint(mp) + 104)]
    assert by(ep.id) == [(len(empty) - 9, 9), (len(empty) - 36, 32)]

    def one(pack, pid, hint_=None, size=None):
        r = Repo({pid: pack})
        return read_headers(key, [(pid, hint_, len(pack) if size is None else size)],
                            r.read_partial, device=None)[0]

    # length + 4 > pack size
    big = good[:-4] + (len(good) - 3).to_bytes(4, "little")
    e = one(big, gp.id)
    assert isinstance(e, RusticError) and e.kind == ErrorKind.Internal
    assert f"Read header length `{len(good) - 3}` + `4` is larger than `{len(good)}`!" in str(e)
    # a MAC failure
    flipped = bytearray(good)
    flipped[-10] ^= 1
    e = one(bytes(flipped), gp.id, hint(gp))
    assert isinstance(e, RusticError) and e.kind == ErrorKind.Cryptography and MAC_MESSAGE in str(e)
    # a type byte above 3
    bad, bp = make_pack(key, [0, 2], "bad", header=run([0]) + b"\x04" + run([2])[1:])
    e = one(bad, bp.id)
    assert isinstance(e, RusticError) and e.kind == ErrorKind.Internal and READ_MESSAGE in str(e)
    # a cut entry
    cut, cp = make_pack(key, [0, 2], "cut", header=run([0, 2], [60, 63])[:-1])
    e = one(cut, cp.id)
    assert isinstance(e, RusticError) and e.kind == ErrorKind.Internal and CONTENTS_MESSAGE in str(e)
    # a wrong pack size: one byte more in front of the pack
    e = one(b"x" + good, gp.id, hint(gp))
    assert isinstance(e, RusticError) and e.kind == ErrorKind.Internal
    assert (f"pack size `{len(good)}` computed from header doesn't match real pack file size "
            f"`{len(good) + 1}`!") in str(e)
    # errors come per pack, the others are read
    r = Repo({gp.id: bytes(flipped), tp.id: tree})
    res = read_headers(key, [(gp.id, None, len(good)), (tp.id, None, len(tree))], r.read_partial,
                       device=None)
    assert isinstance(res[0], RusticError) and res[1].index_pack.blobs == tp.blobs


def test_repair_index_host():
    from rustic_core_amd.errors import RusticError
    from rustic_core_amd.headers import repair_index
    from rustic_core_amd.index import IndexFile, IndexPack
    key = HostKey()
    made = [make_pack(key, t, n) for n, t in
            (("p0", [0, 2, 0]), ("p1", [1, 3]), ("p2", [2] * 4), ("p3", [0]), ("p4", [3, 3, 1]))]
    bad, bp = make_pack(key, [0, 0], "corrupt", header=run([0]) + b"\xff" * 37)
    repo = Repo({p.id: f for f, p in made + [(bad, bp)]})
    ips = [p for _, p in made]
    timed = lambda p: IndexPack(p.id, p.blobs, time="2024-01-02T03:04:05+00:00")
    wrong = IndexPack(ips[2].id, ips[2].blobs[:-1])              # its size is not the pack's
    ghost = _index_pack("ghost")                                  # no such pack
    files = [(bid("index:0"), IndexFile([timed(ips[0]), wrong, ghost])),
             (bid("index:1"), IndexFile([timed(ips[1])])),         # stays as it is
             (bid("index:2"), IndexFile([ips[0], IndexPack(bp.id, bp.blobs)], [timed(ips[3])]))]
    # ips[4] is listed only; ips[0] is indexed twice; the corrupt pack's index entry has the right size

    def run_it(**kw):
        saved, removed = [], []

        def save(f):
            saved.append(f)
            return hashlib.sha256(f.to_json()).digest()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            rep = repair_index(key, files, repo.listed(), repo.read_partial, save, removed.append,
                               device=None, **kw)
        return rep, saved, removed, w

    rep, saved, removed, w = run_it()
    assert rep.modified == [bid("index:0"), bid("index:2")] == removed
    assert rep.dropped == [ghost.id, ips[0].id]
    assert rep.read == [ips[2].id, ips[4].id] and rep.failed == []
    # index:0 without the wrong and the ghost pack; index:2 without the second p0; then the headers read
    assert [f.packs for f in saved] == [[timed(ips[0])], [IndexPack(bp.id, bp.blobs)],
                                        [ips[2], ips[4]]]
    assert saved[1].packs_to_delete == [timed(ips[3])] and not saved[2].packs_to_delete
    assert rep.saved == [hashlib.sha256(f.to_json()).digest() for f in saved]

    rep, saved, removed, w = run_it(read_all=True)
    assert rep.modified == [i for i, _ in files] == removed
    assert rep.read == [ips[0].id, ips[2].id, ips[1].id, ips[3].id, ips[4].id]
    assert [i for i, _ in rep.failed] == [bp.id] and isinstance(rep.failed[0][1], RusticError)
    assert any(bp.id.hex() in str(x.message) for x in w)
    # nothing is left of any index file; everything readable is indexed anew, no time, no mark
    assert len(saved) == 1 and saved[0].packs == [ips[0], ips[2], ips[1], ips[3], ips[4]]
    assert not saved[0].packs_to_delete

    rep2, saved, removed, _ = run_it(read_all=True, dry_run=True)
    assert saved == [] and removed == [] and rep2.saved == []
    assert (rep2.modified, rep2.read, [i for i, _ in rep2.failed]) == \
        (rep.modified, rep.read, [bp.id])
