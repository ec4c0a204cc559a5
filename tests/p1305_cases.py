"""Poly1305 with Python integers, and the crafted keys and messages that the
host tests (test_p1305_host.py), the oracle's pin (test_crypto_oracle.py) and
the device tests (test_gpu_aead_edges.py) share: inputs that random data never
gives -- an unreduced sum in [2^130 - 5, 2^130), limbs of all ones, r of 0, 1,
a single bit and the largest clamped value, at the lengths where the device
kernel changes path."""
import functools

import numpy as np

P = (1 << 130) - 5
CLAMP = 0x0ffffffc0ffffffc0ffffffc0fffffff
M26 = (1 << 26) - 1
M128 = (1 << 128) - 1


def le128(v):
    return int(v).to_bytes(16, "little")


def clamp(r16):
    """r as Poly1305 uses it: top 4 bits of bytes 3, 7, 11, 15 and low 2 of 4, 8, 12 clear."""
    return int.from_bytes(r16, "little") & CLAMP


def limbs(v):
    """v < 2^130 in canonical 26-bit limbs."""
    assert 0 <= v < 1 << 130
    return [(v >> (26 * k)) & M26 for k in range(5)]


def value(h):
    return sum(int(x) << (26 * k) for k, x in enumerate(h))


def poly_sum(r, msg):
    """The unreduced Horner sum over the 16-byte blocks, kept below 2 p only
    by reducing after each step -- returns (h mod p)."""
    h = 0
    for i in range(0, len(msg), 16):
        blk = msg[i:i + 16]
        h = (h + int.from_bytes(blk, "little") + (1 << (8 * len(blk)))) * r % P
    return h


def tag(r16, s, msg):
    """Poly1305 of msg under the 16 key bytes r16 (clamped here) plus s."""
    return le128((poly_sum(clamp(r16), msg) + s) & M128)


# ---- keys ---------------------------------------------------------------------
R_ONE, R_TWO, R_FOUR, R_ZERO = le128(1), le128(2), le128(4), le128(0)
R_MAX = le128(CLAMP)                 # the largest clamped r
R_FF = b"\xff" * 16                  # unclamped: must act as R_MAX
R_TOP = le128(1 << 124)              # only clamped-away bits: acts as 0
R_HIGH = le128(0x0ffffffc0ffffffc0ffffffc00000000)  # low limb 0, the rest at their largest
R_EDGE = [("max", R_MAX), ("ff", R_FF), ("top", R_TOP), ("high", R_HIGH), ("zero", R_ZERO),
          ("one", R_ONE), ("four", R_FOUR)]

# ---- (a) the final reduction window ---------------------------------------------
Z16 = bytes(16)


def reduction_cases():
    """(name, r16, message, unreduced sum): sums at and around p and 2^130.
    With r = 1 the sum is that of the blocks, each plus 2^128."""
    out = []
    for t in range(5):  # p + t: the final subtraction fires, tag = s + t
        out.append((f"p+{t}", R_ONE, le128((1 << 128) - 5 + t) + Z16 + Z16, P + t))
    out.append(("2^130-2", R_ONE, b"\xff" * 32, (1 << 130) - 2))
    out.append(("2^130-2 by r=2", R_TWO, b"\xff" * 16, (1 << 130) - 2))
    out.append(("p-1 by r=2", R_TWO, b"\xfd" + b"\xff" * 15, P - 1))   # the branch not taken
    out.append(("p-1", R_ONE, le128((1 << 128) - 6) + Z16 + Z16, P - 1))
    for t in (0, 1, 2, 5, 6, 7):  # through 2^130: folded by the carry pass's wrap
        out.append((f"2^130-1+{t}", R_ONE, b"\xff" * 16 + le128(t) + Z16, (1 << 130) - 1 + t))
    for name, r16, msg, total in out:  # the construction is what it says
        r, acc = clamp(r16), 0
        for i in range(0, len(msg), 16):
            acc = (acc + int.from_bytes(msg[i:i + 16], "little") + (1 << 128)) * r
        assert acc == total and poly_sum(r, msg) == total % P, name
    return out


# ---- (b) largest limbs: lengths and fills -----------------------------------------
UNIT = 4096 * 16  # bytes of one unit of the device kernel (kAeadUnitBlocks blocks)
LENGTHS = [1, 15, 16, 17, 63 * 16, 64 * 16, 65 * 16, 127 * 16 + 5, 128 * 16, 129 * 16,
           4095 * 16, UNIT, UNIT + 1, 4097 * 16, 2 * UNIT + 63 * 16 + 7, 3 * UNIT]
FILLS = ("ff", "00", "random")


@functools.lru_cache(maxsize=None)
def fill(kind, n):
    if kind == "random":
        return np.random.default_rng(0x1305 + n).integers(0, 256, n, dtype=np.uint8).tobytes()
    return bytes([int(kind, 16)]) * n


def limb_cases():
    """(name, r16, message) for every edge key, fill and length."""
    return [(f"{rn}/{f}/{n}", r16, fill(f, n)) for rn, r16 in R_EDGE for f in FILLS
            for n in LENGTHS]


def mac_cases():
    """Every (name, r16, message) of the lists above."""
    return [(n, r, m) for n, r, m, _ in reduction_cases()] + limb_cases()


@functools.lru_cache(maxsize=None)
def mac_sums():
    """{name: h mod p} of mac_cases(), computed once for every test that asks."""
    return {n: poly_sum(clamp(r), m) for n, r, m in mac_cases()}
