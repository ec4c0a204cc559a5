"""CPU: the family units' planners (csrc/rcdc_family_plans.h), run by
tools/family_plans_check, against Python: pack plans against pack.parse_header
and pack.header_size, the AEAD key material against the oracle's key schedule
and Python integers, and the zstd windows, the decompressor's groups and the
place tiles against a few lines written here from the rules in the header's
comments."""
import base64
import json
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# RCDC_PLANS_CHECK: another build of the same program (one compiled with
# -fsanitize=address,undefined, say) runs the same cases
TOOL = os.environ.get("RCDC_PLANS_CHECK") or os.path.join(ROOT, "tools", "family_plans_check")
KiB, MiB = 1 << 10, 1 << 20
INVALID, UNSUPPORTED = 2, 1


class Toks:
    """One result line: the keyword dropped, ints taken in order."""

    def __init__(self, line):
        self.t, self.i = line.split(), 1

    def one(self):
        self.i += 1
        return int(self.t[self.i - 1])

    def many(self, n):
        return [self.one() for _ in range(n)]

    def rows(self, width):
        return [tuple(self.many(width)) for _ in range(self.one())]

    def done(self):
        return self.i == len(self.t)


@pytest.fixture(scope="module")
def check(rcdc_lib):
    """Feeds the check program cases (token lists); returns per case a Toks,
    or (status, message) for a refused case."""
    assert os.path.exists(TOOL), "tools/family_plans_check not built (csrc/Makefile)"

    def run(cases):
        text = "\n".join(" ".join(str(t) for t in c) for c in cases) + "\n"
        r = subprocess.run([TOOL], input=text, capture_output=True, text=True, check=True)
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        out = []
        for c, ln in zip(cases, lines):
            w = ln.split(" ", 3)
            assert w[0] == c[0]
            out.append((int(w[2]), w[3]) if w[1] == "ERR" else Toks(ln))
        return out
    return run


# ---- pack plans ---------------------------------------------------------------
D_IN = 0x10000


def _src(j):
    return 0x1000000 * (j + 1)


def _pack_case(raw, n_src, out_len, blobs, packs):
    """blobs: (type, len, ulen, in_off, pad); packs: (blob0, nblobs, out_off)."""
    return ["pack", int(raw), n_src, out_len, len(blobs), *[v for b in blobs for v in b],
            len(packs), *[v for p in packs for v in p]]


def _read_batch(t):
    base = t.one()
    blobs = t.rows(8)
    units = t.rows(3)
    unit0 = t.many(t.one())
    return base, blobs, units, unit0


def _words(b16):
    return struct.unpack("<4I", bytes(b16))


def _units(lens):
    """(blob, b0, b1) per 4096 16-byte blocks, and each blob's first unit."""
    units, unit0 = [], []
    for i, n in enumerate(lens):
        unit0.append(len(units))
        nb = (n + 15) // 16
        units += [(i, b0, min(nb, b0 + 4096)) for b0 in range(0, nb, 4096)]
    return units, unit0


def _check_pack(t, raw, n_src, blobs, packs):
    from rustic_core_amd.pack import header_size, parse_header
    assert t.one() == 0
    hdr = bytes(t.many(t.one()))
    offs = t.many(t.one())
    outs = t.rows(2)
    data = _read_batch(t)
    heads = _read_batch(t)
    copies = t.many(t.one())
    assert t.done()
    assert hdr[-4:] == b"\0" * 4  # the padding the kernel may read
    h0, want_data, want_heads, want_copies, want_offs = 0, [], [], [], {}
    for p, ((blob0, nb, out_off), (header_len, size)) in enumerate(zip(packs, outs)):
        mine = blobs[blob0:blob0 + nb]
        sealed = [ln if raw else ln + 32 for _, ln, _, _, _ in mine]
        hlen = sum(41 if u else 37 for _, _, u, _, _ in mine)
        entries = parse_header(hdr[h0:h0 + hlen])
        assert header_size(entries) == hlen
        assert [(e.type, e.offset, e.length, e.uncompressed_len, e.id) for e in entries] == [
            (tp, sum(sealed[:k]), sealed[k], u, bytes((31 * (blob0 + k) + j) & 255 for j in range(32)))
            for k, (tp, _, u, _, _) in enumerate(mine)]
        assert (header_len, size) == (hlen + 32, sum(sealed) + hlen + 32 + 4)
        for k, (tp, ln, u, in_off, pad) in enumerate(mine):
            i, off = blob0 + k, sum(sealed[:k])
            want_offs[i] = off
            if raw:
                base = _src(pad) if n_src else D_IN
                for c in range(0, ln, MiB):
                    want_copies += [in_off + c, out_off + off + c, min(MiB, ln - c), base]
            else:
                want_data.append((in_off, ln, out_off + off,
                                  *_words((i + 3 * j) & 255 for j in range(16)), 0))
        want_heads.append((h0, hlen, out_off + sum(sealed),
                           *_words((5 * p + j + 1) & 255 for j in range(16)), 1))
        h0 += hlen
    assert len(hdr) == h0 + 4
    for i, off in want_offs.items():
        assert offs[i] == off
    assert copies == want_copies
    assert data == (_src(0) if n_src else D_IN, want_data, *_units([b[1] for b in want_data]))
    assert heads == (0, want_heads, *_units([h[1] for h in want_heads]))


def test_pack_plans(check):
    mixed = [(0, 100, 0, 0, 0), (1, 5000, 12000, 128, 0), (0, 70000, 0, 8192, 0),
             (1, 1, 0, 90000, 0), (0, 65536 * 2 + 1, 999999, 100000, 0)]
    cases = [
        (False, 0, 1 << 20, [(0, 1000, 0, 64, 0)], [(0, 1, 16)]),                  # one blob
        (False, 0, 1 << 22, mixed, [(0, 5, 0)]),                                   # data + tree
        (False, 0, 1 << 22, mixed, [(0, 2, 0), (2, 3, 1 << 20)]),                  # two packs
        (True, 0, 1 << 20, [(0, 32, 0, 5, 0)], [(0, 1, 0)]),                       # raw, 32 bytes
        (True, 0, 1 << 22, [(1, MiB + 1, 77, 3, 0)], [(0, 1, 9)]),                 # two copy units
        (True, 3, 1 << 22, [(0, 40, 0, 0, 2), (0, 50, 9, 7, 0), (1, 60, 0, 9, 1)],  # multi-source
         [(0, 2, 0), (2, 1, 4096)]),
    ]
    for c, t in zip(cases, check([_pack_case(*c) for c in cases])):
        _check_pack(t, c[0], c[1], c[3], c[4])
    # the raw blob of 1 MiB + 1: a unit of 1 MiB and one of a byte
    t = check([_pack_case(*cases[4])])[0]
    t.i = len(t.t) - 9
    assert t.many(9) == [8, 3, 9, MiB, D_IN, 3 + MiB, 9 + MiB, 1, D_IN]


def test_pack_plans_refused(check):
    one = [(0, 100, 0, 0, 0)]
    size = 100 + 32 + 37 + 32 + 4
    got = check([
        _pack_case(False, 0, 1 << 20, one, [(0, 0, 0)]),
        _pack_case(False, 0, 1 << 20, one * 3, [(1, 3, 0)]),
        _pack_case(False, 0, 1 << 20, [(2, 100, 0, 0, 0)], [(0, 1, 0)]),
        _pack_case(True, 0, 1 << 20, [(0, 31, 0, 0, 0)], [(0, 1, 0)]),
        _pack_case(False, 0, 64 + size - 1, one, [(0, 1, 64)]),
        _pack_case(True, 3, 1 << 20, [(0, 40, 0, 0, 3)], [(0, 1, 0)]),
    ])
    assert got == [
        (INVALID, "pack 0: blobs [0, +0) of 1"),
        (INVALID, "pack 0: blobs [1, +3) of 3"),
        (INVALID, "blob 0: type 2"),
        (INVALID, "blob 0: 31 sealed bytes (< 32)"),
        (INVALID, f"pack 0 does not fit the output (64 + {size} > {64 + size - 1})"),
        (INVALID, "blob 0: source 3 of 3"),
    ]
    ok = check([_pack_case(False, 0, 64 + size, one, [(0, 1, 64)])])[0]  # exactly fits
    assert ok.one() == 0


# ---- key material ---------------------------------------------------------------
P1305 = (1 << 130) - 5


def _sbox():
    """FIPS-197 5.1.1: the inverse in GF(2^8), then the affine map."""
    def mul(a, b):
        r = 0
        while b:
            if b & 1:
                r ^= a
            a = (a << 1) ^ (0x11b if a & 0x80 else 0)
            b >>= 1
        return r
    sb = []
    for x in range(256):
        inv = next((y for y in range(1, 256) if mul(x, y) == 1), 0)
        rot = lambda v, k: ((v << k) | (v >> (8 - k))) & 255
        sb.append(inv ^ rot(inv, 1) ^ rot(inv, 2) ^ rot(inv, 3) ^ rot(inv, 4) ^ 0x63)
    return sb


def _fixture_key(oracle_mod):
    """The master key of the reference's key file key1 (keys.rs:12-35)."""
    import hashlib
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "crypto_fixtures.json")))["keys_test"]
    kf = json.loads(base64.b64decode(g["key1"]))
    user = hashlib.scrypt(g["passwords"]["key1"].encode(), salt=base64.b64decode(kf["salt"]),
                          n=kf["N"], r=kf["r"], p=kf["p"], maxmem=1 << 30, dklen=64)
    mk = json.loads(oracle_mod.open_(user, base64.b64decode(kf["data"])))
    return (base64.b64decode(mk["encrypt"]) + base64.b64decode(mk["mac"]["k"]) +
            base64.b64decode(mk["mac"]["r"]))


def test_key_material(check, oracle_mod):
    keys = [bytes(64), bytes(range(64)), _fixture_key(oracle_mod)]
    assert len(keys[2]) == 64
    # r at its edges: 0, 1, 2, the largest clamped value, sixteen 0xff bytes (the
    # clamp makes them that value) and only the top nibble (the clamp clears it)
    rmax = 0x0ffffffc0ffffffc0ffffffc0fffffff
    edge = [0, 1, 2, rmax, (1 << 128) - 1, 1 << 124]
    keys += [bytes(range(7, 55)) + v.to_bytes(16, "little") for v in edge]
    clamped = [int.from_bytes(k[48:], "little") & rmax for k in keys[3:]]
    assert clamped == [0, 1, 2, rmax, rmax, 0]
    L = oracle_mod.lib()
    sb = _sbox()
    xt = lambda v: ((v << 1) ^ (0x1b if v & 0x80 else 0)) & 255
    te = [xt(s) << 24 | s << 16 | s << 8 | (xt(s) ^ s) for s in sb]
    val = lambda limbs: sum(v << (26 * k) for k, v in enumerate(limbs)) % P1305
    for key, t in zip(keys, check([["keymat", *key] for key in keys])):
        rk256, rk128 = np.zeros(60, np.uint32), np.zeros(44, np.uint32)
        k256, k128 = np.frombuffer(key[:32], np.uint8), np.frombuffer(key[32:48], np.uint8)
        assert L.crypto_ref_aes_expand(k256.ctypes.data, 8, rk256.ctypes.data) == 14
        assert L.crypto_ref_aes_expand(k128.ctypes.data, 4, rk128.ctypes.data) == 10
        assert t.many(60) == rk256.tolist()
        assert t.many(44) == rk128.tolist()
        # r clamped (Poly1305: top 4 bits of bytes 3, 7, 11, 15 and low 2 of 4, 8, 12 clear)
        r = int.from_bytes(key[48:], "little") & 0x0ffffffc0ffffffc0ffffffc0fffffff
        for i in range(65):
            limbs = t.many(5)
            # table rows are pmul's b operand: every limb below 2^26 (rcdc_p1305.h)
            assert all(v < 1 << 26 for v in limbs) and val(limbs) == pow(r, i, P1305), i
        for j in range(32):
            limbs = t.many(5)
            assert all(v < 1 << 26 for v in limbs) and val(limbs) == pow(r, 1 << j, P1305), j
        assert t.many(256) == te
        assert t.done()


# ---- zstd windows ---------------------------------------------------------------
BLK = 128 * KiB


def _zwin_model(wblocks, lens):
    nblk = lambda n: max((n + BLK - 1) // BLK, 1)
    wins, blobs, blks, i = [], [], [], 0
    while i < len(lens):
        w = [len(blobs), 0, len(blks), 0]
        while i < len(lens) and not (w[3] and w[3] + nblk(lens[i]) > wblocks):
            nb = nblk(lens[i])
            blobs.append((1000 * i, 7 * i, lens[i], w[3], nb))
            blks += [(w[1], k * BLK, min(BLK, lens[i] - k * BLK), (k == 0) | (k + 1 == nb) << 1)
                     for k in range(nb)]
            w[1] += 1
            w[3] += nb
            i += 1
        wins.append(tuple(w))
    return max(w[3] for w in wins), wins, blobs, blks


def test_zstd_windows(check):
    lens = [0, 1, BLK, BLK + 1, 4 * BLK + 1]
    rng = np.random.default_rng(20271)
    cases = [(4, lens), (4, lens[::-1]), (4, [4 * BLK + 1]), (1, lens), (32768, lens),
             (4, [BLK * 2, BLK * 2, 1, BLK * 3 + 1, 0, 0, 0, 0, 0]),
             (7, [int(v) for v in rng.integers(0, 6 * BLK, 60)])]
    for (wb, ls), t in zip(cases, check([["zwin", wb, len(ls), *ls] for wb, ls in cases])):
        got = (t.one(), t.rows(4), t.rows(5), t.rows(4))
        assert t.done() and got == _zwin_model(wb, ls), (wb, ls)
    # spelled out: 0, 1, 128 KiB and 128 KiB + 1 bytes fill a window of 4 blocks... the
    # fourth has 2 blocks and opens the next; the blob of 5 blocks has a window of its own
    t = check([["zwin", 4, len(lens), *lens]])[0]
    assert (t.one(), t.rows(4)) == (5, [(0, 3, 0, 3), (3, 1, 3, 2), (4, 1, 5, 5)])
    blobs, blks = t.rows(5), t.rows(4)
    assert [b[3:] for b in blobs] == [(0, 1), (1, 1), (2, 1), (0, 2), (0, 5)]
    assert blks[0] == (0, 0, 0, 3) and blks[2] == (2, 0, BLK, 3)  # one block: first and last
    assert blks[3:5] == [(0, 0, BLK, 1), (0, BLK, 1, 2)]           # window 1 counts from 0
    assert [b[3] for b in blks[5:]] == [1, 0, 0, 0, 2] and blks[-1] == (0, 4 * BLK, 1, 2)


# ---- the decompressor's groups -----------------------------------------------------
def _zdx_model(ws_max, frames):
    """frames: (need, nblk, status, flags, ncomp, ntreeless, frame_len)."""
    up = lambda v: (v + 255) & ~255
    total = lambda nblk, data: up(up(up(nblk * 48) + nblk * 16) + data)
    groups, place, i = [], [], 0
    while i < len(frames):
        a, nblk, data = i, 0, 0
        while i < len(frames):
            need = 0 if frames[i][2] else frames[i][0]
            if i > a and (data + need > ws_max or nblk + frames[i][1] > 1 << 31):
                break
            place.append((nblk, data))
            nblk += frames[i][1]
            data += need
            i += 1
        groups.append((a, i, nblk, data, total(nblk, data)))
    lists, st = [], [0, 0, 0]
    for a, b, *_ in groups:
        fr = frames[a:b]
        ok = [j for j, f in enumerate(fr) if not f[2]]
        lst = [j for j in ok if fr[j][3] & 1]
        st[1] += sum(fr[j][4] for j in lst)
        st[0] += sum(fr[j][4] for j in ok if j not in lst)
        st[2] += sum(fr[j][5] for j in ok if j not in lst)
        lists.append((lst, sorted(range(b - a), key=lambda j: -fr[j][6])))  # (stable)
    return max(g[4] for g in groups), groups, place, lists, st


def test_zdx_groups(check):
    f = lambda need, nblk=1, status=0, flags=0, flen=100: (need, nblk, status, flags, 3, 1, flen)
    rng = np.random.default_rng(20272)
    cases = [
        (1000, [f(400), f(600), f(1)]),            # exactly the cap, then one more byte
        (1000, [f(400), f(601), f(1)]),            # one above the cap
        (1000, [f(10), f(5000, 9), f(10)]),        # a frame above the cap: its own group
        (1000, [f(5000)]),
        (1000, [f(900), f(900, 4, status=2), f(100), f(1)]),  # refused: needs 0, keeps its slots
        (1000, [f(300, flags=1, flen=5), f(300, flen=9), f(300, flags=1, flen=9), f(300, status=1)]),
        (4 << 30, [f(int(n), int(b), int(s), int(g), int(l)) for n, b, s, g, l in zip(
            rng.integers(0, 1 << 30, 80), rng.integers(1, 9000, 80), rng.integers(0, 3, 80) // 2,
            rng.integers(0, 8, 80), rng.integers(1, 50, 80))]),
    ]
    outs = check([["zdx", ws, len(fr), *[v for x in fr for v in x]] for ws, fr in cases])
    for (ws, fr), t in zip(cases, outs):
        peak, groups, place = t.one(), t.rows(5), t.rows(2)
        lists = [(t.many(t.one()), t.many(t.one())) for _ in groups]
        got = (peak, groups, place, lists, t.many(3))
        assert t.done() and got == _zdx_model(ws, fr), (ws, fr)
    t = check([["zdx", 1000, 3, *[v for x in cases[0][1] for v in x]]])[0]
    assert [g[:4] for g in (t.one(), t.rows(5))[1]] == [(0, 2, 2, 1000), (2, 3, 1, 1)]
    t = check([["zdx", 1000, 4, *[v for x in cases[4][1] for v in x]]])[0]
    t.one()
    assert [g[:4] for g in t.rows(5)] == [(0, 3, 6, 1000), (3, 4, 1, 1)]
    assert t.rows(2) == [(0, 0), (1, 900), (5, 900), (0, 0)]


# ---- place tiles -----------------------------------------------------------------
TILE = 64 * KiB
IN0, OUT0, OUT1 = 0x7f0000000000, 0x7e0000000000, 0x7d0000000010


def _place_case(zero_test, R, ins, outs, blobs, dests, dump=True):
    """ins / outs: (base, len); blobs: (in_off, len, src, dest0, ndests); dests: (out_off, dst)."""
    flat = lambda rows: [v for r in rows for v in r]
    return ["place", int(zero_test), R, len(ins), *flat(ins), len(outs), *flat(outs),
            len(blobs), *flat(blobs), len(dests), *flat(dests), int(dump)]


def _place_model(zero_test, R, ins, outs, blobs, dests):
    tiles = []
    for i, (in_off, ln, src, d0, nd) in enumerate(blobs):
        if not ln or (not zero_test and not nd):
            continue
        s = ins[src][0] + in_off
        al = int(all((outs[dests[d][1]][0] + dests[d][0] - s) % 16 == 0 for d in range(d0, d0 + nd)))
        tiles += [(s + c, min(TILE, ln - c), i, d0, nd, c, al) for c in range(0, ln, TILE)]
    wins, pos, w0, w, rnd, k = [], 0, 0, 4096, 0, 0
    for _ in tiles:  # windows of 4096, 8192, ... tiles; R tiles a round
        if pos == R:
            if pos > w0:
                wins.append((rnd, k, pos - w0))
                w *= 2
            pos, w0, k, rnd = 0, 0, 0, rnd + 1
        pos += 1
        if pos - w0 >= w:
            wins.append((rnd, k, pos - w0))
            w0, w, k = pos, w * 2, k + 1
    if pos > w0:
        wins.append((rnd, k, pos - w0))
    return rnd, wins, tiles


def test_place_tiles(check):
    ins, outs = [(IN0, 1 << 30)], [(OUT0, 1 << 30), (OUT1, 1 << 30)]
    blobs = [(0, 0, 0, 0, 1), (16, 1, 0, 1, 1), (4096, TILE, 0, 2, 2), (100000, TILE + 1, 0, 4, 1),
             (300000, 5000, 0, 5, 0),       # no destination: only the zero test sees it
             (400000, 3 * TILE, 0, 5, 1),   # congruent to its source mod 16
             (400016, 3 * TILE, 0, 6, 2)]   # one of its two destinations is not
    dests = [(0, 0), (32, 0), (8192, 0), (8192 - 16, 1), (7, 0), (400000 + 1024, 0),
             (16, 0), (17, 0)]
    cases = [(zt, R, ins, outs, blobs, dests) for zt in (True, False) for R in (1 << 20, 2, 3)]
    for c, t in zip(cases, check([_place_case(*c) for c in cases])):
        assert t.one() == 0
        got = (t.one(), t.rows(3), t.rows(7))
        assert t.done() and got == _place_model(*c), c[:2]
    t = check([_place_case(*cases[0])])[0]
    t.many(2)
    t.rows(3)
    tiles = t.rows(7)
    assert [x[1] for x in tiles if x[2] == 3] == [TILE, 1] and [x[1] for x in tiles if x[2] == 1] == [1]
    assert {x[2]: x[6] for x in tiles} == {1: 1, 2: 1, 3: 0, 4: 1, 5: 1, 6: 0}
    assert 4 not in {x[2] for x in _place_model(*cases[3])[2]}  # without the zero test
    # a tile cap of 2: the blob of 3 tiles straddles two rounds
    r2 = _place_model(*cases[1])
    assert r2[0] >= 2 and all(n <= 2 for _, _, n in r2[1])


def test_place_windows_grow(check):
    """4097 tiles from the enumerator alone (no data behind the addresses): a
    window of 4096, then the rest in the window of 8192."""
    n = 4097
    ins, outs = [(IN0, n * TILE)], [(OUT0, n * TILE)]
    lens = [TILE] * 4000 + [97 * TILE]
    blobs = [(sum(lens[:i]), ln, 0, i, 1) for i, ln in enumerate(lens)]
    dests = [(b[0], 0) for b in blobs]
    c = (True, 1 << 20, ins, outs, blobs, dests)
    t = check([_place_case(*c, dump=False)])[0]
    assert t.many(2) == [0, 0] and t.rows(3) == [(0, 0, 4096), (0, 1, 1)] and t.done()
    assert _place_model(*c)[1] == [(0, 0, 4096), (0, 1, 1)]
    n = 4096 + 8192 + 1  # one blob, from the second of two sources: three windows
    t = check([_place_case(True, 1 << 20, [(IN0, 0), (IN0, n * TILE)], [(OUT0, n * TILE)],
                           [(0, n * TILE, 1, 0, 1)], [(0, 0)], dump=False)])[0]
    assert t.many(2) == [0, 0] and t.rows(3) == [(0, 0, 4096), (0, 1, 8192), (0, 2, 1)]


def test_place_refused(check):
    ins, outs = [(IN0, 1000)], [(OUT0, 1000)]
    got = check([
        _place_case(True, 8, ins, outs, [(0, 10, 1, 0, 0)], []),
        _place_case(True, 8, ins, outs, [(991, 10, 0, 0, 0)], []),
        _place_case(True, 8, ins, outs, [(0, 10, 0, 0, 2)], [(0, 0)]),
        _place_case(True, 8, ins, outs, [(0, 10, 0, 0, 1)], [(0, 1)]),
        _place_case(True, 8, ins, outs, [(0, 10, 0, 0, 1)], [(991, 0)]),
        _place_case(True, 8, [(0, 1000)], outs, [(0, 10, 0, 0, 0)], []),
    ])
    assert got == [
        (INVALID, "blob 0: src 1 >= n_ins 1"),
        (INVALID, "blob 0: in_off 991 + len 10 > in_lens[0] = 1000"),
        (INVALID, "blob 0: dest0 0 + ndests 2 > ndests_total 1"),
        (INVALID, "blob 0, dest 0: dst 1 >= n_outs 1"),
        (INVALID, "blob 0, dest 0: out_off 991 + len 10 > out_lens[0] = 1000"),
        (INVALID, "blob 0: d_ins[0] is NULL"),
    ]
