"""CPU: rustic_core_amd.check with ``device=None`` -- the plain-Python rule
the device path is held against -- against the reference's own recorded
results (tests/golden/check_fixtures.json, check_n_m.json), and the model of
rcdc_check_packs' rule (tests/ckpack_model.py) against that rule and against
read.check_pack's sort.  Opening is the oracle's and zstd is libzstd here."""
import datetime
import random

import numpy as np
import pytest

from tests import ckpack_model as cm
from tests.check_cases import INACTIVE, N_M, REPOS, normal, recorded, run
from tests.test_used_blobs_host import OracleKey


def _now(s):
    return datetime.datetime.fromisoformat(s).replace(tzinfo=datetime.timezone.utc)


def test_parse_n_m_recorded_pairs():
    """All 18 spellings at the 7 dates: 126 recorded pairs."""
    from rustic_core_amd.check import ReadSubset, parse_n_m
    assert len(N_M["cases"]) == 18 and len(N_M["dates"]) == 7
    seen = 0
    for spelling, pairs in N_M["cases"].items():
        n, m = spelling.split("/")
        for date, want in zip(N_M["dates"], pairs):
            assert list(parse_n_m(_now(date), n, m)) == want, (spelling, date)
            assert ReadSubset.parse(spelling, _now(date)) == ReadSubset("IdSubSet", tuple(want))
            seen += 1
    assert seen == 126


def test_parse_spellings_and_errors():
    from rustic_core_amd.check import ReadSubset
    from rustic_core_amd.errors import ErrorKind, RusticError
    assert ReadSubset.parse("all") == ReadSubset("All")
    assert ReadSubset.parse("5%") == ReadSubset("Percentage", 5.0)
    assert ReadSubset.parse("2.5%") == ReadSubset("Percentage", 2.5)
    assert ReadSubset.parse("250MiB") == ReadSubset("Size", 250 << 20)
    assert ReadSubset.parse("1GB") == ReadSubset("Size", 10 ** 9)
    assert ReadSubset.parse("1.5 KiB") == ReadSubset("Size", 1536)
    assert ReadSubset.parse("77") == ReadSubset("Size", 77)
    assert ReadSubset.parse("29/28") == ReadSubset("IdSubSet", (1, 28))
    for bad in ("x%", "a/b", "3/0", "-1/5", "weekly/week", "12 parsecs", ""):
        with pytest.raises(RusticError) as e:
            ReadSubset.parse(bad)
        assert e.value.kind == ErrorKind.InvalidInput


def _test_packs(rng, count=500, pack_size=100_000_000):
    from rustic_core_amd.index import IndexPack
    return [IndexPack(bytes(rng.getrandbits(8) for _ in range(32)), [], None,
                      rng.randrange(pack_size)) for _ in range(count)]


def test_n_m_partitions_500_ids():
    from rustic_core_amd.check import ReadSubset
    packs = _test_packs(random.Random(5))
    left = {p.id for p in packs}
    assert len(left) == 500
    now = _now("2024-10-11T12:00:00")
    for s in ("1/5", "2/5", "3/5", "4/5", "5/5"):
        for p in ReadSubset.parse(s, now).apply(packs):
            left.remove(p.id)  # KeyError: a pack in two parts
    assert not left


@pytest.mark.parametrize("s", ["all", "5/12", "5%", "250MiB"])
def test_subset_sizes(s):
    """The inequalities of the reference's test_read_subset; its StdRng
    sequence is not reproduced, so which packs are chosen is not compared."""
    from rustic_core_amd.check import ReadSubset
    rng = random.Random(5)
    packs = _test_packs(rng)
    size = lambda ps: sum(p.pack_size() for p in ps)
    total = size(packs)
    subset = ReadSubset.parse(s, _now("2024-10-11T12:00:00"))
    got = subset.apply(packs, rng)
    if subset.kind == "All":
        assert size(got) == total and got == packs
    elif subset.kind == "Percentage":
        assert size(got) <= int(total * subset.value)
        assert 0 < size(got) <= int(total * subset.value / 100.0)
    elif subset.kind == "Size":
        assert size(got) <= subset.value <= size(got) + 100_000_000
    else:
        n, m = subset.value
        assert got == [p for p in packs if int.from_bytes(p.id[:4], "little") % m == n % m]
        assert 0 < len(got) < 500


def test_saturating_retain_rule():
    """A pack is kept while the size left is larger than it (not equal), and
    a pack that does not fit does not end the pass."""
    from rustic_core_amd.check import ReadSubset
    from rustic_core_amd.index import IndexPack

    class Fixed(random.Random):
        def shuffle(self, x):
            pass
    packs = [IndexPack(bytes([i]) * 32, [], None, s) for i, s in enumerate([100, 100, 500, 50, 49])]
    got = ReadSubset("Size", 250).apply(packs, Fixed())
    assert [p.size for p in got] == [100, 100, 49]  # 250 -> 150 -> 50; 50 is not > 50; 49 fits
    assert ReadSubset("Percentage", float("nan")).apply(packs, Fixed()) == []
    assert ReadSubset("Percentage", -3.0).apply(packs, Fixed()) == []
    assert ReadSubset("Percentage", 1e30).apply(packs, Fixed()) == packs


@pytest.mark.parametrize("name", REPOS)
def test_fixture_results(oracle_mod, name):
    """check_repository(device=None, read_data=True) gives exactly the
    recorded findings: kind and fields, check_packs' findings in the recorded
    order and the later passes' behind them.  repo-index-missing-blob's
    snapshot is from a test the reference has switched off: the one inactive
    case; it pins ``file: "home/thinkpad/data/test"``."""
    got = normal(run(name, oracle_mod, lambda master: OracleKey(oracle_mod, master), None))
    assert got == recorded(name)
    if name == INACTIVE:
        assert got[-1][2]["file"] == "home/thinkpad/data/test"


def test_results_is_ok(oracle_mod):
    from rustic_core_amd.errors import ErrorKind, RusticError
    key = lambda master: OracleKey(oracle_mod, master)
    run("repo-duplicates.tar.gz", oracle_mod, key, None).is_ok()
    run("repo-unreferenced-data.tar.gz", oracle_mod, key, None).is_ok()  # a warning only
    with pytest.raises(RusticError) as e:
        run("repo-data-missing.tar.gz", oracle_mod, key, None).is_ok()
    assert e.value.kind == ErrorKind.Repository and "check found errors!" in str(e.value)


def _index_pack(ids, locs, types, pid=b"\x07" * 32):
    from rustic_core_amd.index import IndexPack
    p = IndexPack(pid)
    for i, l, t in zip(ids, locs, types):
        p.add(bytes(i), int(t), int(l[1]), int(l[2]), int(l[3]) or None)
    return p


def test_model_against_host_rule_and_check_pack_sort():
    """The model's findings are index_pass_host's, and its order is the order
    read.check_pack sorts the index blobs into wherever that one is decided
    by the location (its further keys, type and id, only order equal
    locations)."""
    from rustic_core_amd.check import index_pass_host
    from rustic_core_amd.read import _ulen
    rng = np.random.default_rng(11)
    for count, shuffle, gap in [(0, False, False), (1, False, False), (2, True, False),
                                (50, False, True), (63, True, True), (200, True, False)]:
        ids, locs, types = cm.random_pack(rng, count, shuffle, gap)
        if count > 3:
            types[rng.integers(0, count, 3)] = 1
            locs[count // 3, 2] = 0xFFFFFFF0  # the running offset wraps
        packs, findings, order = cm.model(ids, locs, types, [(0, count)], 1 << 20)
        p = _index_pack(ids, locs, types)
        want = index_pass_host(p)
        assert len(want) == len(findings) == packs[0]["type_findings"] + packs[0]["offset_findings"]
        for (_, e, kind, got, expected), (level, f) in zip(findings, want):
            assert level == "Error" and f.fields["blob_id"] == bytes(ids[e])
            if kind == cm.TYPE:
                assert (f.kind, f.fields["blob_type"], f.fields["expected"]) == \
                    ("PackBlobTypesMismatch", got, expected)
            else:
                assert (f.kind, f.fields["offset"], f.fields["expected"]) == \
                    ("PackBlobOffsetMismatch", got, expected)
        assert packs[0]["header_len"] == 32 + sum(41 if l[3] else 37 for l in locs)
        by_check_pack = sorted(p.blobs, key=lambda b: (b.offset, b.length, _ulen(b), b.type, b.id))
        assert [(b.offset, b.length, _ulen(b)) for b in by_check_pack] == \
            [tuple(int(x) for x in locs[order[k]][1:]) for k in range(count)]
        if len({tuple(l[1:]) for l in locs}) == count:
            assert [b.id for b in by_check_pack] == [bytes(ids[order[k]]) for k in range(count)]


def test_model_tie_rule_and_host_status():
    """Equal locations keep input order; a pack out of order above the sort's
    capacity is the host's and leaves the numbering of the others alone."""
    ids = np.arange(6 * 32, dtype=np.uint8).reshape(6, 32)
    locs = np.array([[0, 0, 40, 0], [0, 40, 40, 0], [0, 40, 40, 0], [0, 0, 40, 0], [0, 80, 40, 0],
                     [0, 0, 40, 0]], np.uint32)
    packs, findings, order = cm.model(ids, locs, None, [(0, 6)], 8)
    assert [order[k] for k in range(6)] == [0, 3, 5, 1, 2, 4]
    assert [(e, got, exp) for _, e, _, got, exp in findings] == \
        [(3, 0, 40), (5, 0, 80), (1, 40, 120), (2, 40, 160), (4, 80, 200)]
    packs, findings, order = cm.model(ids, locs, None, [(4, 2), (0, 4), (4, 0)], 3)
    assert [p["status"] for p in packs] == [cm.OK, cm.HOST, cm.OK]
    assert packs[0]["sorted"] == 0 and packs[1]["first_finding"] == 0 and 0 not in order
    # pack 0 sorts to entries 5, 4: offset 80 where 40 is expected
    assert findings == [(0, 4, cm.OFFSET, 80, 40)] and packs[2]["first_finding"] == 1


def test_check_packs_lists_and_time():
    """PackTimeNotSet for packs to delete, the hot list and the pack list."""
    from rustic_core_amd.check import check_packs
    from rustic_core_amd.index import IndexFile, IndexPack
    a, b, c, d = (bytes([i]) * 32 for i in (4, 3, 2, 1))
    f = IndexFile()
    pa, pb = IndexPack(a), IndexPack(b, time="2024-01-01T00:00:00Z")
    pa.add(b"\x10" * 32, 1, 0, 50)
    pb.add(b"\x11" * 32, 0, 0, 60)
    pc = IndexPack(c)
    pc.add(b"\x12" * 32, 1, 0, 70)
    f.add(pa)
    f.add(pb, delete=True)
    f.add(pc, delete=True)
    found, collected, missing = check_packs([f], [(a, pa.pack_size()), (b, 1), (d, 5)],
                                            [(d, 5), (b, 2), (c, 1)], device=None)
    assert collected == [pa] and missing == {c: (pc.pack_size(), True)}
    assert [(lv, x.kind, x.fields.get("id")) for lv, x in found] == [
        ("Error", "PackTimeNotSet", c), ("Warn", "HotPackNotReferenced", d),
        ("Warn", "HotDataPack", b), ("Error", "HotPackSizeMismatchIndex", c),
        ("Error", "NoHotPack", a), ("Warn", "PackNotReferenced", d),
        ("Error", "PackSizeMismatchIndex", b), ("Error", "NoPack", c)]


def test_node_name_and_tree_nodes():
    from rustic_core_amd.check import _join, node_name
    from rustic_core_amd.tree import parse_tree_nodes_host
    assert node_name("plain") == "plain" and node_name("a\\\\b") == "a\\b"
    assert node_name("t\\x41\\u00e4\\n") == "tAä\n" and node_name("bad\\q") == "bad\\q"
    assert _join("", "a") == "a" and _join("a/b", "c") == "a/b/c"
    text = (b'{"nodes":[{"name":"f","type":"file"},{"name":"d","type":"dir"},'
            b'{"name":"g","type":"file","content":["' + b"00" * 32 + b'"]}]}')
    nodes = parse_tree_nodes_host(text)
    assert [(n.name, n.type, n.content, n.subtree) for n in nodes] == \
        [("f", "file", None, None), ("d", "dir", None, None), ("g", "file", [bytes(32)], None)]
