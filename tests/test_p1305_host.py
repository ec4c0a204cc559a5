"""CPU: the Poly1305 limb arithmetic of csrc/rcdc_p1305.h -- the code the AEAD
kernels run -- compiled for the host in tools/family_plans_check and compared
with Python integers, at the entry bounds the header states and at the values
random data never reaches: sums at p and 2^130, limbs of all ones, the final
conditional subtraction.  Every assertion is exact: the value mod 2^130 - 5,
and the exit limb bounds written in the header."""
import itertools

import numpy as np
import pytest

from tests.p1305_cases import M26, M128, P, le128, limbs, value
from tests.test_family_plans_host import check  # noqa: F401  (the fixture; RCDC_PLANS_CHECK)

# rcdc_p1305.h, "The limb contracts in one place"
A_BOUND = 1 << 28          # pmul: limbs of a
B_BOUND = 1 << 26          # pmul: limbs of b (the rpow and r2j tables)
PMUL_H1 = (1 << 26) + (1 << 7)
N_BOUND = 1 << 31          # pnorm, pfull: limbs on entry


def _pmul_ok(a, b, got):
    assert value(got) % P == value(a) * value(b) % P, (a, b, got)
    assert all(got[k] < 1 << 26 for k in (0, 2, 3, 4)) and got[1] < PMUL_H1, (a, b, got)


def _run_pmul(check, pairs):
    outs = check([["pmul", *a, *b] for a, b in pairs])
    for (a, b), t in zip(pairs, outs):
        got = t.many(5)
        assert t.done()
        _pmul_ok(a, b, got)
    return len(pairs)


A_EDGE = [0, 1, M26, 1 << 26, A_BOUND - 1]
B_EDGE = [0, 1, M26, B_BOUND - 1]  # (the table bound is 2^26: its largest limb is M26)


def test_pmul_edge_limbs(check):
    """Every edge value of a limb of a against every edge value of a limb of
    b: all five limbs equal, and one limb at a time (the others 0, or the
    others at the largest value)."""
    def spellings(v, rest):
        return [[v] * 5] + [[v if k == j else rest for k in range(5)] for j in range(5)]
    a_all = [s for v in A_EDGE for rest in (0, A_BOUND - 1) for s in spellings(v, rest)]
    b_all = [s for v in B_EDGE for rest in (0, B_BOUND - 1) for s in spellings(v, rest)]
    uniq = lambda rows: [list(r) for r in sorted({tuple(r) for r in rows})]
    pairs = list(itertools.product(uniq(a_all), uniq(b_all)))
    assert _run_pmul(check, pairs) > 1000


def test_pmul_corners_and_max(check):
    """The 1024 combinations of (limb of a in {0, max}) x (limb of b in {0,
    max}); all-max x all-max is among them: the five 64-bit sums at the stated
    bound (21 * (2^28 - 1) * (2^26 - 1) each, plus the carries)."""
    amax, bmax = A_BOUND - 1, B_BOUND - 1
    pairs = [([amax * ((i >> k) & 1) for k in range(5)], [bmax * ((j >> k) & 1) for k in range(5)])
             for i in range(32) for j in range(32)]
    assert pairs[-1] == ([amax] * 5, [bmax] * 5)
    assert _run_pmul(check, pairs) == 1024


def test_pmul_random(check):
    """20 000 seeded pairs inside the contract; half with a's limbs drawn near
    the bound (the top bits set), so carries run long."""
    rng = np.random.default_rng(0x26)
    a = rng.integers(0, A_BOUND, (20000, 5))
    b = rng.integers(0, B_BOUND, (20000, 5))
    a[::2] |= rng.integers(0, 2, (10000, 5)) * (3 << 26)
    b[::4] |= rng.integers(0, 2, (5000, 5)) * (0x3ff << 16)
    assert a.max() < A_BOUND and b.max() < B_BOUND
    _run_pmul(check, [(x.tolist(), y.tolist()) for x, y in zip(a, b)])


# ---- pnorm, pfull ------------------------------------------------------------------
def _spellings(v):
    """Limb vectors of the value v (below 2^131 + 8), each limb below 2^31: the
    lower four limbs canonical and the top one holding the rest; one limb
    borrowed into the limb below (h[j+1] - 1, h[j] + 2^26) at every position it
    can be; and the top limb with 1, 2 or 31 more multiples of 2^130 (the value
    then stands for v + e 2^130)."""
    base = [(v >> (26 * k)) & M26 for k in range(4)] + [v >> 104]
    out = [(list(base), v)]
    for j in range(4):
        if base[j + 1]:
            h = list(base)
            h[j + 1] -= 1
            h[j] += 1 << 26
            out.append((h, v))
    if all(base[j + 1] for j in range(4)):  # every limb borrowed into at once
        h = list(base)
        for j in range(4):
            h[j + 1] -= 1
            h[j] += 1 << 26
        out.append((h, v))
    for e in (1, 2, 31):
        h = list(base)
        h[4] += e << 26
        if h[4] < N_BOUND:
            out.append((h, v + (e << 130)))
    assert all(value(h) == val and max(h) < N_BOUND for h, val in out)
    return out


def _near():
    vals = set()
    for c in (0, P, 1 << 130, 2 * P, 1 << 131):
        vals.update(v for v in range(c - 8, c + 9) if v >= 0)
    return [s for v in sorted(vals) for s in _spellings(v)]


def _limb_edges():
    """Entry-bound limbs: all at the bound, one at the bound, and all ones."""
    top = N_BOUND - 1
    rows = [[top] * 5, [M26] * 5, [1 << 26] * 5, [0] * 5]
    rows += [[top if k == j else 0 for k in range(5)] for j in range(5)]
    rows += [[top if k == j else M26 for k in range(5)] for j in range(5)]
    return [(h, value(h)) for h in rows]


def test_pnorm(check):
    cases = _near() + _limb_edges()
    assert any(h[4] >> 26 == 31 for h, _ in cases)
    for (h, val), t in zip(cases, check([["pnorm", *h] for h, _ in cases])):
        got = t.many(5)
        assert value(got) % P == val % P, (h, got)
        # exit: h1 <= 2^26, the others < 2^26
        assert all(got[k] < 1 << 26 for k in (0, 2, 3, 4)) and got[1] <= 1 << 26, (h, got)


def test_pfull(check):
    cases = _near() + _limb_edges()
    rng = np.random.default_rng(0x27)
    cases += [(h, value(h)) for h in rng.integers(0, N_BOUND, (2000, 5)).tolist()]
    for (h, val), t in zip(cases, check([["pfull", *h] for h, _ in cases])):
        got = t.many(5)
        assert value(got) % P == val % P, (h, got)
        assert all(x < 1 << 26 for x in got) and value(got) < 1 << 130, (h, got)
    # what the tag step relies on: values in [p, 2^130) stay as they are
    t = check([["pfull", *limbs(P + 3)]])[0]
    assert t.many(5) == limbs(P + 3)


# ---- ptag ---------------------------------------------------------------------------
def test_ptag(check):
    """h around p (the conditional subtraction taken from p on, not at p - 1),
    up to 2^130 - 1, and the 64- and 128-bit seams of joining the limbs; s at
    the carries of the 128-bit addition."""
    hs = list(range(P - 8, P + 5)) + list(range((1 << 130) - 8, 1 << 130))
    hs += [0, 1, (1 << 64) - 1, 1 << 64, (1 << 128) - 1]
    assert P + 4 == (1 << 130) - 1 and all(P - 8 <= h < 1 << 130 for h in hs[:-5])
    ss = [0, 1, (1 << 64) - 1, 1 << 64, M128, (1 << 128) - (1 << 64)]
    cases = list(itertools.product(hs, ss))
    outs = check([["ptag", *limbs(h), s & ((1 << 64) - 1), s >> 64] for h, s in cases])
    for (h, s), t in zip(cases, outs):
        got = bytes(t.many(16))
        assert t.done() and got == le128((h % P + s) & M128), (h, s, got.hex())
    # the subtraction matters: for h = p + t the tag without it would be 5 less
    t = check([["ptag", *limbs(P + 2), 7, 0]])[0]
    assert bytes(t.many(16)) == le128(9)


# ---- pblock -------------------------------------------------------------------------
def test_pblock(check):
    """Every byte count 0..16 of a block of 0xff (bytes at and after k must
    not leak into the value; the 2^(8 k) bit where it belongs, also at the
    word seams k = 4, 8, 12 and at 16), of zeros (the bit alone) and of
    distinct bytes."""
    words = lambda b: [int.from_bytes(b[i:i + 4], "little") for i in (0, 4, 8, 12)]
    blocks = [b"\xff" * 16, bytes(16), bytes(range(0x81, 0x91))]
    cases = [(b, k) for b in blocks for k in range(17)]
    for (b, k), t in zip(cases, check([["pblock", *words(b), k] for b, k in cases])):
        got = t.many(5)
        want = int.from_bytes(b[:k], "little") + (1 << (8 * k))
        assert got == limbs(want), (b.hex(), k, got)
        assert got[4] < 1 << 25
