"""CPU: the ingest engine's pure steps (csrc/rcdc_ingest_steps.h), run by
tools/ingest_steps_check, against Python: the pack grouping against
pack.group_blobs_open (the model of packer.rs should_save / take_data /
finalize), the pack layout, the D2H grouping and the cut lists against a few
lines written here from the rules in the header's comments."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# RCDC_STEPS_CHECK: another build of the same program (one compiled with
# -fsanitize=address,undefined, say) runs the same cases
TOOL = os.environ.get("RCDC_STEPS_CHECK") or os.path.join(ROOT, "tools", "ingest_steps_check")


@pytest.fixture(scope="module")
def check(rcdc_lib):
    """Feeds the check program cases (token lists), returns a list of int
    lists: one result line per case, the leading keyword dropped."""
    assert os.path.exists(TOOL), "tools/ingest_steps_check not built (csrc/Makefile)"

    def run(cases):
        text = "\n".join(" ".join(str(t) for t in c) for c in cases) + "\n"
        r = subprocess.run([TOOL], input=text, capture_output=True, text=True, check=True)
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        for c, ln in zip(cases, lines):
            assert ln.split()[0] == c[0]
        return [[int(t) for t in ln.split()[1:]] for ln in lines]
    return run


# ---- grouping -------------------------------------------------------------
def _group_case(sizer4, finalize, aged, lens, ulens):
    flat = [v for p in zip(lens, ulens) for v in p]
    return ["group", *sizer4, int(finalize), int(aged), len(lens), *flat]


def _group_result(out):
    n = out[0]
    packs = [(out[1 + 2 * i], out[2 + 2 * i]) for i in range(n)]
    return packs, out[1 + 2 * n], out[2 + 2 * n]


def _model(sizer4, finalize, lens, ulens):
    """group_blobs_open takes the blobs' lengths before sealing."""
    from rustic_core_amd.pack import PackSizer, group_blobs_open
    s = PackSizer(sizer4[0], sizer4[1], sizer4[2], sizer4[3], 30, 300)
    packs, open_from = group_blobs_open([n - 32 for n in lens], s, ulens, finalize=finalize)
    return [(int(a), int(b)) for a, b in packs], int(open_from), int(s.current_size)


def _random_group_cases():
    rng = np.random.default_rng(20261)
    k = int(rng.integers(1 << 10, 1 << 22))
    currents = [0, 1, 1 << 20, k * k - 1, k * k, (1 << 44) - 1, 1 << 44]
    cases = []
    for i in range(240):
        default = int(rng.choice([4 << 10, 64 << 10, 1 << 20]))
        grow = int(rng.choice([0, 1, 32, 1000]))
        limit = int(rng.choice([default // 3, default - 1, default + 1, 16 * default, 0xFFFFFFFF]))
        current = int(rng.choice(currents)) if i % 3 else int(rng.integers(0, 1 << 44))
        n = int(rng.integers(0, 400))
        if i % 8 == 0:  # small blobs: MAX_COUNT closes packs before the size does
            lens = rng.integers(33, 41, 25000 if i == 0 else n * 60)
            default, limit = 1 << 20, 0xFFFFFFFF
        else:
            lens = rng.integers(33, int(rng.choice([200, 5000, 200000])), n)
        ulens = np.where(rng.random(len(lens)) < 0.7, lens * 2, 0)
        cases.append(((default, grow, limit, current), bool(i & 1), [int(v) for v in lens],
                      [int(v) for v in ulens]))
    cases.append(((1 << 20, 32, 0xFFFFFFFF, 0), True, [], []))   # an empty list
    cases.append(((1 << 20, 32, 0xFFFFFFFF, 0), False, [], []))
    return cases


def test_grouping_matches_the_python_packer(check):
    cases = _random_group_cases()
    outs = check([_group_case(s, fin, False, lens, ulens) for s, fin, lens, ulens in cases])
    closed_by_count = 0
    for (s, fin, lens, ulens), out in zip(cases, outs):
        got = _group_result(out)
        assert got == _model(s, fin, lens, ulens), (s, fin, len(lens))
        closed_by_count += sum(1 for _, n in got[0] if n == 10000)
    assert closed_by_count >= 2  # the 10 000-blob rule was exercised


def test_grouping_sqrt_at_square_minus_one(check):
    """pack_size() at current = k^2 - 1 takes isqrt = k - 1 (std::sqrt on a
    double against math.isqrt), up to 2^44."""
    cases = []
    for k in (2, 3, 1000, (1 << 16) + 1, (1 << 22) - 1, 1 << 22):
        for cur in (k * k - 1, k * k):
            # one blob just below / at the limit the Python sizer gives
            limit = (math.isqrt(cur) * 1000 + 4096) & 0xFFFFFFFF
            for ln in (limit - 1, limit):
                cases.append(((4096, 1000, 0xFFFFFFFF, cur), False, [ln], [0]))
    outs = check([_group_case(s, fin, False, lens, ulens) for s, fin, lens, ulens in cases])
    for (s, fin, lens, ulens), out in zip(cases, outs):
        assert _group_result(out) == _model(s, fin, lens, ulens), (s, lens)


def test_grouping_in_two_calls_equals_one(check):
    """The open pack of the first call leads the second (the engine's carry
    across batches): packs, and the sizer, as in one call."""
    rng = np.random.default_rng(20262)
    for _ in range(12):
        lens = [int(v) for v in rng.integers(33, 60000, int(rng.integers(50, 300)))]
        ulens = [int(v) * int(rng.integers(0, 2)) for v in lens]
        cut = int(rng.integers(0, len(lens) + 1))
        s = (256 << 10, 32, 0xFFFFFFFF, int(rng.integers(0, 1 << 30)))
        one = _group_result(check([_group_case(s, True, False, lens, ulens)])[0])
        p1, open1, cur1 = _group_result(check([_group_case(s, False, False, lens[:cut],
                                                           ulens[:cut])])[0])
        p2, open2, cur2 = _group_result(check([_group_case((s[0], s[1], s[2], cur1), True, False,
                                                           lens[open1:], ulens[open1:])])[0])
        assert open2 == len(lens) - open1
        assert (p1 + [(a + open1, n) for a, n in p2], cur2) == (one[0], one[2])
        assert one == _model(s, True, lens, ulens)


def test_grouping_aged(check):
    """`aged` with a non-empty list: the first pack closes even below the
    limit; nothing else changes."""
    rng = np.random.default_rng(20263)
    for i in range(20):
        n = int(rng.integers(1, 200))
        lens = [int(v) for v in rng.integers(33, 9000, n)]
        ulens = [int(v) * (i & 1) for v in lens]
        s = (int(rng.choice([64 << 10, 4 << 20])), 32, 0xFFFFFFFF, 0)
        plain, aged = (_group_result(o) for o in check([_group_case(s, False, False, lens, ulens),
                                                        _group_case(s, False, True, lens, ulens)]))
        if plain[0]:  # the first pack closed by size anyway
            assert aged == plain
            continue
        # nothing closed without it: with it, all of the list is the one pack,
        # the sizer takes its size, and nothing is left open
        hdr = sum(41 if u else 37 for u in ulens)
        assert aged == ([(0, n)], n, s[3] + sum(lens) + hdr + 32 + 4)
    # aged closes only the first pack: what follows it stays open as without
    lens, ulens, s = [40000, 40000, 100], [0, 0, 0], (64 << 10, 0, 0xFFFFFFFF, 0)
    plain, aged = (_group_result(o) for o in check([_group_case(s, False, False, lens, ulens),
                                                    _group_case(s, False, True, lens, ulens)]))
    assert plain == aged == ([(0, 2)], 2, 80000 + 74 + 36)


# ---- layout and D2H grouping ------------------------------------------------
def test_layout_and_d2h_groups(check):
    rng = np.random.default_rng(20264)
    for _ in range(20):
        n = int(rng.integers(1, 300))
        lens = [int(v) for v in rng.integers(33, 70000, n)]
        ulens = [int(v) * int(rng.integers(0, 2)) for v in lens]
        # groups: consecutive, the first at 0, an open rest left out
        bounds = sorted(set(int(v) for v in rng.integers(1, n + 1, int(rng.integers(1, 12)))))
        groups = [(a, b - a) for a, b in zip([0] + bounds[:-1], bounds)]
        flat = [v for p in zip(lens, ulens) for v in p]
        out = check([["layout", n, *flat, len(groups), *[v for g in groups for v in g]]])[0]
        # a pack: its blobs, a header entry each (41 compressed, 37 stored),
        # 32 B of header sealing and the u32; packs back to back
        sizes = [sum(lens[a:a + k]) + sum(41 if u else 37 for u in ulens[a:a + k]) + 36
                 for a, k in groups]
        offs = [sum(sizes[:j]) for j in range(len(sizes))]
        assert out == [sum(sizes)] + [v for p in zip(offs, sizes) for v in p]
        total = sum(sizes)
        for gb in (1, 70000, 300000, 1 << 40):
            got = check([["d2h", gb, total, len(offs), *offs]])[0]
            # whole packs until the group spans gb bytes, one pack at least
            want, a = [], 0
            while a < len(offs):
                b = a + 1
                while b < len(offs) and offs[b] - offs[a] < gb:
                    b += 1
                want += [a, b, offs[a], offs[b] if b < len(offs) else total]
                a = b
            assert got == [len(want) // 4] + want
            if gb == 1:
                assert got[0] == len(offs)
            if gb == 1 << 40:
                assert got == [1, 0, len(offs), 0, total]
    assert check([["d2h", 1, 0, 0]])[0] == [0]
    assert check([["layout", 0, 0]])[0] == [0]


# ---- cut lists ------------------------------------------------------------
def _cuts_model(max_chunk, units):
    """units: (stream, final, aborted, off, len, cslot, cuts)."""
    ncuts, chunks, carries, copies = [], [], [], []
    for i, (stream, final, aborted, off, ln, cslot, cuts) in enumerate(units):
        keep = list(cuts)
        if stream and (not final or aborted):  # the last chunk is not final
            keep = keep[:-1]
            start = keep[-1] if keep else 0
            if not aborted:                    # it is the carry (an aborted stream has none)
                carries += [i, start]
                if ln > start:
                    copies += [off + start, cslot * max_chunk, ln - start]
        ncuts.append(len(keep))
        prev = 0
        for c in keep:
            chunks += [c, off + prev, c - prev]
            prev = c
    return ([len(units)] + ncuts + [len(chunks) // 3] + chunks + [len(carries) // 2] + carries +
            [len(copies) // 3] + copies)


def _cuts_case(max_chunk, units):
    flat = []
    for stream, final, aborted, off, ln, cslot, cuts in units:
        flat += [int(stream), int(final), int(aborted), off, ln, cslot, len(cuts), *cuts]
    return ["cuts", max_chunk, len(units), *flat]


def test_cut_lists(check):
    mc = 8192
    whole = (False, True, False, 256, 10000, 0, [3000, 7000, 10000])
    open_stream = (True, False, False, 16384, 9000, 3, [2000, 6000, 9000])
    final_stream = (True, True, False, 32768, 5000, 1, [4000, 5000])
    aborted = (True, True, True, 49152, 5000, 2, [4000, 5000])
    no_chunks = (True, False, False, 65536, 0, 5, [])
    one_chunk = (True, False, False, 81920, 700, 4, [700])  # all of it is the carry
    empty_file = (False, True, False, 98304, 0, 0, [])
    units = [whole, open_stream, final_stream, aborted, no_chunks, one_chunk, empty_file]
    cases = [[u] for u in units] + [units, units[::-1], []]
    outs = check([_cuts_case(mc, c) for c in cases])
    for c, out in zip(cases, outs):
        assert out == _cuts_model(mc, c), c
    # spelled out once: the open stream's last chunk is its carry, not a chunk
    assert outs[1] == [1, 2, 2, 2000, 16384, 2000, 6000, 18384, 4000, 1, 0, 6000,
                       1, 16384 + 6000, 3 * mc, 3000]
    assert outs[3] == [1, 1, 1, 4000, 49152, 4000, 0, 0]       # aborted: no carry
    assert outs[4] == [1, 0, 0, 1, 0, 0, 0]                    # zero chunks: an empty carry
    rng = np.random.default_rng(20265)
    rand = []
    for _ in range(30):
        us, off = [], 0
        for _ in range(int(rng.integers(0, 12))):
            cuts = sorted(set(int(v) for v in rng.integers(1, 50000, int(rng.integers(0, 9)))))
            ln = cuts[-1] if cuts else 0
            stream = bool(rng.integers(0, 2))
            final = bool(rng.integers(0, 2)) or not stream
            us.append((stream, final, stream and final and bool(rng.integers(0, 2)), off, ln,
                       int(rng.integers(0, 16)), cuts))
            off += (ln + 255) // 256 * 256
        rand.append(us)
    for c, out in zip(rand, check([_cuts_case(mc, c) for c in rand])):
        assert out == _cuts_model(mc, c), c
