"""Blob encryption on the device at the edges of its Poly1305 (rcdc_aead.hip
over rcdc_p1305.h): keys and ciphertexts crafted so that the unreduced sum
lands at p, at 2^130 and around them, limbs are all ones, r is 0, 1, a single
bit or the largest clamped value, and blobs end where the kernel changes path.
Random keys and data (test_gpu_aead.py) reach none of this: the final
conditional subtraction alone has a chance of 2^-127 per blob.

Method: the test chooses all 64 key bytes, so r is chosen.  The MAC runs over
the ciphertext: for open the test supplies it; for seal it takes the keystream
from the oracle (zeros sealed under the same key and nonce) and submits
plaintext = wanted ciphertext XOR keystream.  The expected tag is Poly1305 in
Python integers (tests/p1305_cases.py) plus s = AES-128_k(nonce) from the
oracle, cross-checked against the oracle's whole sealed blob on every case
(the oracle's Poly1305 is pinned on the same cases in test_crypto_oracle.py).
Every case goes both ways: seal gives nonce || ct || tag byte for byte, open of
that blob gives status 0 and the plaintext, open with the tag plus 1 gives
status 1.  All assertions are exact."""
import hashlib

import numpy as np
import pytest

from oracle import oracle
from tests.p1305_cases import (FILLS, LENGTHS, M128, P, R_EDGE, R_MAX, R_ONE, UNIT, clamp, fill,
                               le128, mac_sums, poly_sum, reduction_cases)

pytestmark = pytest.mark.gpu

ENC = bytes((37 * i + 11) & 255 for i in range(32))   # the AES-256 key
KK = bytes((101 * i + 7) & 255 for i in range(16))    # Poly1305-AES's k


def _key(r16):
    return ENC + KK + r16


def _nonce(name):
    return hashlib.sha256(name.encode()).digest()[:16]


def _s(nonce):
    return int.from_bytes(oracle.aes_encrypt_block(KK, nonce), "little")


def _xor(a, b):
    return (np.frombuffer(a, np.uint8) ^ np.frombuffer(b, np.uint8)).tobytes()


def _plain_for(key, nonce, ct):
    """The plaintext whose ciphertext under (key, nonce) is ct."""
    ks = oracle.seal(key, nonce, bytes(len(ct)))[16:16 + len(ct)]
    return _xor(ct, ks)


def _layout(lens, mult, phase):
    """Offsets at least 16 bytes apart, blob i misaligned by (mult i + phase) mod 16."""
    offs, o = [], 0
    for i, n in enumerate(lens):
        o = (o + 15) // 16 * 16 + 16 + (mult * i + phase) % 16
        offs.append(o)
        o += n
    return offs, (o + 15) // 16 * 16 + 64


def _run(key, items, seal, nonces=None):
    """One device batch over `items` (plaintexts to seal, or sealed blobs to
    open), inputs and outputs at every misalignment 0..15, the output filled
    with 0xA5 first: returns the outputs (and the statuses of an open) and
    checks that nothing between the outputs was written."""
    import torch
    from rustic_core_amd.crypto import Key, make_refs
    in_lens = [len(b) for b in items]
    out_lens = [n + 32 if seal else max(n - 32, 0) for n in in_lens]
    in_offs, in_total = _layout(in_lens, 1, 0)
    out_offs, out_total = _layout(out_lens, 5, 3)
    assert len(items) < 16 or ({o % 16 for o in in_offs} == {o % 16 for o in out_offs} ==
                               set(range(16)))
    arena = np.zeros(in_total, np.uint8)
    for o, b in zip(in_offs, items):
        arena[o:o + len(b)] = np.frombuffer(b, np.uint8)
    d_in = torch.from_numpy(arena).to("cuda:0")
    d_out = torch.full((out_total,), 0xA5, dtype=torch.uint8, device="cuda:0")
    k = Key(key)
    st = None
    if seal:
        k.seal_blobs(d_in.data_ptr(), make_refs(in_offs, in_lens, out_offs, b"".join(nonces)),
                     d_out.data_ptr())
    else:
        st = k.open_blobs(d_in.data_ptr(), make_refs(in_offs, in_lens, out_offs),
                          d_out.data_ptr()).tolist()
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    gaps = np.ones(out_total, bool)
    for o, n in zip(out_offs, out_lens):
        gaps[o:o + n] = False
    assert np.all(out[gaps] == 0xA5), "bytes written outside the blobs"
    return [out[o:o + n].tobytes() for o, n in zip(out_offs, out_lens)], st


def _bump(blob, delta=1):
    """The sealed blob with its tag plus delta (mod 2^128)."""
    t = (int.from_bytes(blob[-16:], "little") + delta) & M128
    return blob[:-16] + le128(t)


def _both_ways(r16, cases, forged=()):
    """cases: (name, wanted ciphertext, h mod p).  forged: (case index, tag
    delta) of further blobs that open must refuse."""
    key = _key(r16)
    nonces = [_nonce(n) for n, _, _ in cases]
    plains = [_plain_for(key, nc, ct) for nc, (_, ct, _) in zip(nonces, cases)]
    want = [nc + ct + le128((h + _s(nc)) & M128) for nc, (_, ct, h) in zip(nonces, cases)]
    for (name, _, _), nc, pt, w in zip(cases, nonces, plains, want):
        assert oracle.seal(key, nc, pt) == w, name  # integers and the oracle agree
    got, _ = _run(key, plains, True, nonces)
    for (name, _, _), g, w in zip(cases, got, want):
        assert g[:16] == w[:16] and g[16:-16] == w[16:-16], f"{name}: nonce or ciphertext"
        assert g[-16:] == w[-16:], f"{name}: tag {g[-16:].hex()} != {w[-16:].hex()}"
    blobs = want + [_bump(w) for w in want] + [_bump(want[i], d) for i, d in forged]
    n = len(want)
    outs, st = _run(key, blobs, False)
    assert st[:n] == [0] * n, [c[0] for c, s in zip(cases, st) if s]
    assert outs[:n] == plains
    assert st[n:] == [1] * (len(blobs) - n), "a wrong tag was accepted"


# ---- (a) the final reduction window --------------------------------------------------
def test_final_reduction_window(gpu_ctx):
    """Unreduced sums p + t (t = 0..4: the final subtraction fires, tag = s +
    t), 2^130 - 2 with and without a multiplication, p - 1 both ways (the branch
    not taken) and 2^130 - 1 + t (folded by the carry pass).  For p + t the tag
    a kernel without the final subtraction would make, s + t - 5, is refused."""
    by_key = {}
    for name, r16, msg, total in reduction_cases():
        by_key.setdefault(r16, []).append((name, msg, total % P, total))
    for r16, rows in by_key.items():
        cases = [(n, m, h) for n, m, h, _ in rows]
        for n, m, h, total in rows:  # the tag is s + (total mod p)
            if n.startswith("p+"):
                assert h == int(n[2:]) and P <= total < 1 << 130
        forged = [(i, -5) for i, (n, _, _, _) in enumerate(rows) if n.startswith("p+")]
        assert r16 != R_ONE or len(forged) == 5
        _both_ways(r16, cases, forged)


# ---- (b) largest limbs -----------------------------------------------------------------
@pytest.mark.parametrize("rname", [n for n, _ in R_EDGE])
def test_largest_limbs(gpu_ctx, rname):
    """One edge key; fills of 0xff, 0x00 and seeded random bytes at 16 lengths:
    one lane, a full row of lanes, the second block of the two-block step
    present and absent, a unit exactly full, a unit of one block, one and two
    units after the first (r^(2^j) positioning), a partial last block."""
    r16 = dict(R_EDGE)[rname]
    sums = mac_sums()
    cases = [(f"{rname}/{f}/{n}", fill(f, n), sums[f"{rname}/{f}/{n}"]) for f in FILLS
             for n in LENGTHS]
    assert len(cases) == 48 and max(len(c[1]) for c in cases) == 3 * UNIT
    if rname in ("zero", "top"):  # r = 0 after the clamp: the tag is s alone
        assert clamp(r16) == 0 and all(h == 0 for _, _, h in cases)
    _both_ways(r16, cases)


# ---- (c) adding s -----------------------------------------------------------------------
# fixed once; the assertions below hold for these under KK
S_NONCES = [bytes.fromhex(h) for h in ("00000000000000000000000000000000",
                                       "000102030405060708090a0b0c0d0e0f",
                                       "ffffffffffffffffffffffffffffffff",
                                       "a5a5a5a5a5a5a5a55a5a5a5a5a5a5a5a")]


def test_adding_s(gpu_ctx):
    """r = 1 and one block: h = ct + 2^128 is chosen, and the tag is (ct + s)
    mod 2^128.  ct of all ones, of a low half of all ones and of zeros under
    four nonces each; and, from each nonce's s, the four ciphertexts that put
    the sum exactly at and one below each carry: low half into high half, and
    out of 2^128."""
    key = _key(R_ONE)
    m64 = (1 << 64) - 1
    cases, low3, top3 = [], set(), set()
    for k, nc in enumerate(S_NONCES):
        s = _s(nc)
        cts = [M128, m64, 0,
               ((1 << 128) - s) & M128,              # ct + s = 2^128: tag 0
               (M128 - s) & M128,                    # ct + s = 2^128 - 1: tag of all ones
               ((1 << 64) - (s & m64)) & m64,        # the low halves sum to 2^64
               m64 - (s & m64)]                      # ... to 2^64 - 1
        low = [(ct & m64) + (s & m64) > m64 for ct in cts]
        top = [ct + s > M128 for ct in cts]
        # a change of key cannot hollow the cases out: under every nonce each
        # carry happens and is absent, and over the nonces so it is for the
        # first three ciphertexts alone
        assert set(low) == set(top) == {False, True}, nc.hex()
        assert (top[3], top[4], low[5], low[6]) == (True, False, True, False), nc.hex()
        low3.update(low[:3])
        top3.update(top[:3])
        for j, ct in enumerate(cts):
            h = ct + (1 << 128)
            assert h < P and poly_sum(1, le128(ct)) == h
            cases.append((f"s{k}/{j}", le128(ct), h))
    assert low3 == top3 == {False, True}
    # the cases run under their own nonces (s belongs to the nonce)
    nonces = [S_NONCES[int(n[1])] for n, _, _ in cases]
    plains = [_plain_for(key, nc, ct) for nc, (_, ct, _) in zip(nonces, cases)]
    want = [nc + ct + le128((h + _s(nc)) & M128) for nc, (_, ct, h) in zip(nonces, cases)]
    for nc, pt, w in zip(nonces, plains, want):
        assert oracle.seal(key, nc, pt) == w
    assert want[3][-16:] == bytes(16) and want[4][-16:] == b"\xff" * 16
    got, _ = _run(key, plains, True, nonces)
    assert got == want
    outs, st = _run(key, want + [_bump(w) for w in want] + [_bump(w, -1) for w in want], False)
    n = len(want)
    assert st == [0] * n + [1] * (2 * n) and outs[:n] == plains


# ---- (d) tag comparison and message coverage -------------------------------------------
def test_every_tag_byte_and_message_end_is_checked(gpu_ctx):
    """One sealed blob of two units plus a partial block, opened 36 times in
    one batch: untouched; each tag byte in turn XOR 0x01, then XOR 0x80; a flip
    in the first block of the second unit, in the last byte of the partial
    block, and in the first byte after the nonce."""
    key = _key(R_MAX)
    n = 2 * UNIT + 7
    data = fill("random", n)
    sealed = oracle.seal(key, _nonce("coverage"), data)
    assert len(sealed) == n + 32

    def flip(pos, bit):
        b = bytearray(sealed)
        b[pos] ^= bit
        return bytes(b)
    blobs = [sealed]
    blobs += [flip(16 + n + j, 0x01) for j in range(16)]
    blobs += [flip(16 + n + j, 0x80) for j in range(16)]
    blobs += [flip(16 + UNIT + 3, 0x10), flip(16 + n - 1, 0x01), flip(16, 0x01)]
    outs, st = _run(key, blobs, False)
    assert st == [0] + [1] * 35
    assert outs[0] == data


# ---- (e) the same kernel through the packer ------------------------------------------------
def test_pack_build_at_the_reduction_window(gpu_ctx):
    """rcdc_pack_build (blobs sealed in place, the header from the staging
    buffer with its length appended) under the r = 1 key, with three blobs whose
    ciphertexts sum to p, p + 4 and 2^130 - 2: the pack equals the oracle's
    byte for byte."""
    import torch
    from rustic_core_amd.pack import build_packs, make_blobs, pack_layout
    key = _key(R_ONE)
    picked = [c for c in reduction_cases() if c[0] in ("p+0", "p+4", "2^130-2")]
    assert len(picked) == 3
    nonces = [_nonce("pack " + c[0]) for c in picked]
    datas = [_plain_for(key, nc, c[2]) for nc, c in zip(nonces, picked)]
    for nc, d, c in zip(nonces, datas, picked):  # the sealed blob carries the crafted tag
        assert oracle.seal(key, nc, d)[-16:] == le128((c[3] % P + _s(nc)) & M128)
    ids = [hashlib.sha256(d).digest() for d in datas]
    hnonce = _nonce("pack header")
    offs, total_in = _layout([len(d) for d in datas], 1, 5)
    arena = np.zeros(total_in, np.uint8)
    for o, d in zip(offs, datas):
        arena[o:o + len(d)] = np.frombuffer(d, np.uint8)
    blobs = make_blobs(offs, [len(d) for d in datas], [np.frombuffer(i, np.uint8) for i in ids],
                       [np.frombuffer(nc, np.uint8) for nc in nonces], types=[0, 1, 0],
                       uncompressed=[0, 0, 0])
    packs, total = pack_layout(blobs, [(0, 3)], [np.frombuffer(hnonce, np.uint8)])
    d_in = torch.from_numpy(arena).to("cuda:0")
    d_out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    offsets = build_packs(gpu_ctx, key, d_in.data_ptr(), blobs, packs, d_out.data_ptr(), total)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    want, index = oracle.pack_file(key, [(t, d, i, nc, 0) for t, d, i, nc in
                                         zip([0, 1, 0], datas, ids, nonces)], hnonce)
    assert int(packs[0]["size"]) == len(want) == total
    assert out[:total].tobytes() == want
    assert [int(o) for o in offsets] == [o for o, _ in index]
    assert np.all(out[total:] == 0xA5)
