"""rcdc_pack_header_parse on the device against the plain-Python model
(tests/pack_header_model.py): the case table, the places where the walk over
tiles can go wrong at the smallest sizes that show them, one long header and
one batch of many, and the reference's own mixed pack through
``headers.read_headers``."""
import numpy as np
import pytest

from oracle import oracle
from tests import pack_header_model as model
from tests.pack_header_cases import (TABLE, phase_walk, random_header, run, sized, sizes_to,
                                     straddle)
from tests.pack_header_model import BAD_TYPE, CUT_SHORT, OK, OVERFLOW

pytestmark = pytest.mark.gpu

GUARD = 64


def _arena(headers, align=1, shift=0):
    """One device arena holding ``headers`` back to back, each at a multiple
    of ``align``, the whole tensor starting ``shift`` bytes past a 16-byte
    boundary; 0xFF wherever no header lies.  Returns (tensor, offs, lens)."""
    offs, o = [], 0
    for h in headers:
        o = (o + align - 1) // align * align
        offs.append(o)
        o += len(h)
    host = np.full(o + shift + 1, 0xFF, np.uint8)
    for off, h in zip(offs, headers):
        host[shift + off:shift + off + len(h)] = np.frombuffer(h, np.uint8)
    return _upload(host, o, shift), offs, [len(h) for h in headers]


def _upload(host, o, shift):
    """``host[shift : shift + o]`` on the device, ``shift`` bytes past a
    16-byte boundary."""
    import torch
    t = torch.from_numpy(host).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    return t[shift:shift + o]


def _check(headers, pack_base=(0, 0), align=1, shift=0, want_ids=(True, True),
           want_locs=(True, True)):
    """Parse ``headers`` in one call and compare every output with the model;
    nothing is written past the counts reported (0xA5 fill and guard)."""
    from rustic_core_amd.headers import PK_HEADER, parse_headers
    d, offs, lens = _arena(headers, align, shift)
    res = parse_headers(d, offs, lens, pack_base, want_ids=want_ids, want_locs=want_locs,
                        guard=GUARD)
    m = model.collect(headers, pack_base)
    names = [n for n in PK_HEADER.names if n != "pad"]
    assert set(names) == set(model.Record._fields)
    _compare(res, {n: np.array([getattr(r, n) for r in m.records], np.int64) for n in names}, m.packs,
             [b"".join(i) for i in m.ids],
             [np.array(l, np.uint32).reshape(-1, 4) for l in m.locs], want_ids, want_locs)
    return res, m


def _compare(res, records, packs, ids, locs, want_ids=(True, True), want_locs=(True, True)):
    """Every output of a call against what is expected: ``records`` an array
    per field of PK_HEADER, ``ids[t]`` the id bytes and ``locs[t]`` (n, 4)
    uint32 per type; behind what was written the 0xA5 fill and guard."""
    for n, want in records.items():
        assert np.array_equal(res.headers[n].astype(np.int64), want), n
    assert res.packs == tuple(packs) and res.entries == tuple(len(i) // 32 for i in ids)
    raw = iter(res.raw)
    for t in (0, 1):
        n = len(ids[t]) // 32
        if want_ids[t]:
            flat = next(raw).cpu().numpy()
            assert flat[:n * 32].tobytes() == ids[t], t
            assert (flat[n * 32:] == 0xA5).all(), t
        else:
            assert res.ids[t] is None
        if want_locs[t]:
            flat = next(raw).cpu().numpy()
            assert np.array_equal(flat[:n * 16].view(np.uint32).reshape(-1, 4), locs[t]), t
            assert (flat[n * 16:] == 0xA5).all(), t
        else:
            assert res.locs[t] is None


def _tile():
    from rustic_core_amd.headers import parse_tile
    return parse_tile()


def test_table_in_one_batch_and_one_by_one(gpu_ctx):
    ok = [c[1] for c in TABLE if c[2] == OK]
    bad = [c[1] for c in TABLE if c[2] != OK]
    turns = []  # accepted and rejected in turns
    for k in range(max(len(ok), len(bad))):
        turns += ok[k:k + 1] + bad[k:k + 1]
    assert len(turns) == len(TABLE)
    res, m = _check(turns, shift=5)  # back to back at odd offsets, off a 16-byte boundary
    assert sorted(set(m.status)) == [OK, BAD_TYPE, CUT_SHORT, OVERFLOW]
    for name, header, status in TABLE:
        _, m = _check([header], shift=3)
        assert m.status == [status], name


def test_a_rejected_header_changes_nothing_of_its_neighbours(gpu_ctx):
    a, b, c = run([0, 2, 0]), run([3, 1]), run([2, 2])
    for bad in (b"\x04" + a[1:], a[:-1], run([0, 0], lengths=[0x80000000] * 2), b"\x00"):
        res, m = _check([a, bad, b, bad, c, bad], shift=1)
        _, m0 = _check([a, b, c], shift=1)
        assert m.ids == m0.ids and m.locs == m0.locs
        assert [r for r in m.records if r.status == OK] == m0.records


def test_one_tile_one_byte_more_one_byte_less(gpu_ctx):
    tile = _tile()
    for n in (tile, tile + 1, tile - 1):
        whole = sized(sizes_to(n))
        assert len(whole) == n
        longer = sized([37] * (n // 37 + 2))[:n]  # that many bytes, the last entry cut
        for h in (whole, longer):
            _check([h], align=16)           # its tiles are the arena's
            _check([h, run([1, 3])], align=1, shift=9)
            _check([run([1]), h, run([0])], align=1, shift=15)


@pytest.mark.parametrize("id_byte", [None, 0xFF, 0x04])
def test_an_entry_straddles_the_boundary_at_every_phase(gpu_ctx, id_byte):
    """With ids of 0xFF or 0x04 every byte off the chain is a bad type byte:
    none of them reaches a status."""
    tile = _tile()
    hs = [straddle(tile, p, id_byte) for p in range(41)]
    assert all(len(h) > tile + 40 for h in hs)
    _, m = _check(hs, align=16)
    assert m.status == [OK] * 41
    _check(hs, align=1, shift=7)


def test_the_phase_changes_in_every_tile(gpu_ctx):
    tile = _tile()
    h = phase_walk(tile, 7)
    assert len({(k * tile) % 37 for k in range(7)}) == 7
    _, m = _check([h], align=16)
    assert m.status == [OK]
    _check([h[:-5], h, h + b"\x07"], shift=11)


def test_a_bad_type_byte_at_a_tiles_first_and_last_byte(gpu_ctx):
    tile = _tile()
    first = sized(sizes_to(tile)) + b"\x09" + run([0])[1:] + run([0, 2])
    last = sized(sizes_to(tile - 1)) + b"\xf0" + run([0])[1:] + run([0, 2])
    _, m = _check([first, last], align=16)
    assert [(r.status, r.err_pos) for r in m.records] == [(BAD_TYPE, tile), (BAD_TYPE, tile - 1)]
    # the same bytes as the last ones of their headers: checked before the size
    _, m = _check([first[:tile + 1], last[:tile]], align=16)
    assert m.status == [BAD_TYPE] * 2
    # and one byte earlier the headers are whole
    _, m = _check([first[:tile], last[:tile - 1]], align=16)
    assert m.status == [OK] * 2


def test_a_last_entry_cut_over_a_tile_boundary(gpu_ctx):
    tile = _tile()
    front = sized(sizes_to(tile - 20))  # the last entry starts 20 bytes before the boundary
    hs = [front + run([3])[:cut] for cut in range(1, 41)]
    _, m = _check(hs, align=16)
    assert [(r.status, r.err_pos) for r in m.records] == [(CUT_SHORT, tile - 20)] * 40
    _check(hs, shift=13)


def test_empty_headers_and_overflow_over_tiles(gpu_ctx):
    _, m = _check([b"", b"", run([1]), b""], (3, 4))
    assert [(r.type, r.number, r.count) for r in m.records] == \
        [(0, 3, 0), (0, 4, 0), (1, 4, 1), (0, 5, 0)]
    _check([b""])
    n = 3 * _tile() // 37
    over = run([0] * n, lengths=[(1 << 32) // n + 1] * n)
    fits = run([0] * n, lengths=[((1 << 32) - 1) // n] * n)
    _, m = _check([over, fits, over], shift=2)
    assert m.status == [OVERFLOW, OK, OVERFLOW]
    assert m.locs[0][-1][1] + m.locs[0][-1][2] <= 0xFFFFFFFF


def _long_header(rng, n, tree=False):
    types = (rng.integers(0, 2, n) * 2 + (1 if tree else 0)).tolist()
    lengths = rng.integers(0, 30000, n).tolist()
    ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return b"".join(model.entry(t, l, i.tobytes(), l + 1 if t >= 2 else 0)
                    for t, l, i in zip(types, lengths, ids))


def test_one_header_of_65535_entries(gpu_ctx):
    """About 2.6 MB: some 1 250 tiles, so the chain goes through many rounds
    of 64 tiles."""
    h = _long_header(np.random.default_rng(3), 65535, tree=True)
    assert len(h) > 64 * 3 * _tile()
    assert len(h) // _tile() > 19 * 64  # twenty rounds of the chain's 64 tiles
    res, m = _check([run([0]), h, run([1, 1])], shift=4)
    assert m.status == [OK] * 3 and m.records[1].count == 65535
    assert [r.number for r in m.records] == [0, 0, 1]


def test_5000_tiny_headers(gpu_ctx):
    """The numbering scan runs over more than one workgroup."""
    rng = np.random.default_rng(8)
    hs = [random_header(rng, n_max=4, bad=0.3) for _ in range(5000)]
    _, m = _check(hs, (7, 1 << 20), shift=6)
    assert min(m.packs) > 1024 and m.status.count(OK) < 4900


def test_more_headers_than_a_round_of_sums(gpu_ctx):
    """2^20 + 2100 headers in one call: 1 027 workgroups number them, so the
    one workgroup over their sums (``block_scan4``) takes a second round with
    a carry.  Empty headers, one data entry, one tree entry, two compressed
    entries, and a bad type byte in every 1 000th header (so before and after
    the 2^20th); every record and both entry arrays are
    ``pack_header_cases.Pattern``'s arithmetic, which
    tests/test_pack_header_host.py holds to the model."""
    from rustic_core_amd.headers import parse_headers
    from tests.pack_header_cases import PATTERN_EVERY, Pattern
    n, base = (1 << 20) + 2100, (7, 1 << 20)
    assert n > 1024 * 1024 and (1 << 20) % PATTERN_EVERY not in (0, PATTERN_EVERY - 1)
    p = Pattern(n, base)
    bad = np.nonzero(p.records["status"])[0]
    assert len(bad) == n // PATTERN_EVERY and bad[-3] < 1 << 20 < bad[-2]
    o, shift = len(p.arena), 6
    host = np.full(o + shift + 1, 0xFF, np.uint8)
    host[shift:shift + o] = p.arena
    res = parse_headers(_upload(host, o, shift), p.offs, p.lens, base, guard=GUARD)
    _compare(res, p.records, p.packs, [i.tobytes() for i in p.ids], p.locs)


def test_pack_base_and_outputs_off(gpu_ctx):
    rng = np.random.default_rng(2)
    hs = [random_header(rng, bad=0.1) for _ in range(40)]
    _check(hs, (1000, 0xFFFF0000))
    for want_ids in ((True, False), (False, True), (False, False)):
        for want_locs in ((True, True), (False, True), (True, False), (False, False)):
            _check(hs, (3, 5), want_ids=want_ids, want_locs=want_locs)


def test_invalid_input(gpu_ctx):
    import torch
    from rustic_core_amd.errors import ErrorKind, RusticError
    from rustic_core_amd.headers import parse_headers
    d, offs, lens = _arena([run([0, 2])])
    with pytest.raises(RusticError) as e:
        parse_headers(d, [offs[0] + 1], lens)  # the ref ends behind the arena
    assert e.value.kind == ErrorKind.InvalidInput
    with pytest.raises(RusticError):
        parse_headers(d.cpu(), offs, lens)
    res = parse_headers(torch.empty(0, dtype=torch.uint8, device="cuda:0"), [], [])
    assert res.entries == (0, 0) and len(res.headers) == 0


def test_the_references_mixed_pack(gpu_ctx):
    """repo-mixed: 1 data blob and 4 tree blobs in one header.  The device
    flags it mixed; read_headers sends it through the host and gives the
    entries of the fixture's own index file."""
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.headers import HeaderResult, read_headers
    from rustic_core_amd.restore import from_packs
    from tests.test_used_blobs_host import fixture
    key, files, index_file, pack_id = fixture(oracle)
    pack = [v for n, v in files.items() if n.startswith("repo/data/")][0]
    whole = index_file.packs[0]
    calls = []

    def read_partial(pack_id_, offset, length):
        calls.append((offset, length))
        return from_packs({pack_id: pack})(pack_id_, offset, length)
    for hint in (None, 32 + 5 * 41, 1000):
        r, = read_headers(Key(key), [(pack_id, hint, len(pack))], read_partial)
        assert isinstance(r, HeaderResult)
        assert (r.data, r.tree, r.mixed, r.count) == (1, 4, True, 5)
        assert r.type == whole.blobs[0].type and r.pack_size == len(pack)
        assert r.index_pack.blobs == whole.blobs and r.index_pack.id == pack_id
        assert int(r.parsed.headers["status"][0]) == OK
    assert len(calls) == 2 + 1 + 1  # a second read only where the guess was too small
