"""Host model of what the walk builds from rcdc_slide.h, against the CPU oracle.

The model restates the device arithmetic, vectorised over lanes as the kernel
is (numpy arrays of 32-bit halves, one element per lane):

* the slide on the OM and MOD tables (`v_alignbit`, the byte insert of
  `v_perm`, the three-input XORs) with each MOD address form: the
  one-instruction `v_lshrrev_b32_sdwa` into byte 1 of a register whose other
  bytes keep the lane's table offset (TSH >= 200), the two-instruction form it
  replaced (TSH 105), and the generic-degree form (TSH < 0);
* `scan_unit` at G = 1016: groups of 16 kept fingerprints, one `v_min_u16` per
  byte over the low halves (non-SMALL, mask >= 0xFFFF) or over `h0 & mask`
  (SMALL), the `acc == 0` gate, and `record_group` with its OR shortcut and
  its `rlo` / `rhi` clipping into first / last / count;
* the min zone's warm-up (`slide_in`).

Every lane owns a segment as in the kernels (64 warm-up bytes, then S tested
positions), and the counted range of each pass is clipped in the middle of a
group.  Cuts built from the model's candidates must equal `oracle.chunk_cuts`
on random data, on zeros and across a zero run shorter than min, at degree 53
and at a generic degree, for both prefilter forms.
"""
import functools

import numpy as np
import pytest

from oracle import oracle

KiB = 1 << 10
TABLE_BYTES = 256 * 32 * 8  # kTableBytes: the MOD table's offset in LDS
S = 1536                    # the walk's segment
G = 16
NONE = 0xFFFFFFFF
GENERIC_POLY = (1 << 40) | 0x1B
NONSMALL = (32 * KiB, 64 * KiB, 512 * KiB)   # mask 0xFFFF
SMALL = (8 * KiB, 8 * KiB, 64 * KiB)         # mask 0x1FFF
U32 = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.uint64(x)


class Lanes:
    """The slide state of n lanes.  form: "sdwa", "bitop3" (degree 53) or
    "generic" (any degree)."""

    def __init__(self, n, poly, form):
        out, mod, deg, _ = oracle.table_arrays(poly)
        assert form == "generic" or deg == 53
        self.deg, self.form = deg, form
        self.mod = mod.astype(np.uint64)
        o = out.astype(np.uint64) << _u(8)
        self.om = o ^ self.mod[((o >> _u(deg)) & _u(255)).astype(np.int64)]  # fill_tables step 2
        lane = np.arange(n, dtype=np.uint64) & _u(63)
        self.lwo = (lane & _u(31)) * _u(8)
        self.lwm = self.lwo | _u(TABLE_BYTES)
        self.ma = self.lwm.copy()          # make_consts: k.ma = k.lwm
        self.sh = _u(deg - 40)             # make_consts: idx_shift - 8
        self.h0 = np.zeros(n, np.uint64)
        self.h1 = np.zeros(n, np.uint64)

    def _lds(self, addr):
        """ds_read_b64 from each lane's own copy (entry e of copy c at e * 256 + c * 8)."""
        table, off = addr // _u(TABLE_BYTES), addr % _u(TABLE_BYTES)
        assert np.all(off % _u(256) == self.lwo) and np.all(table <= 1)
        e = (off // _u(256)).astype(np.int64)
        return np.where(table == 1, self.mod[e], self.om[e])

    def _mod_addr(self):
        if self.form == "sdwa":
            # v_lshrrev_b32_sdwa ma, sh, h1 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE
            byte = ((self.h1 >> self.sh) & U32) & _u(0xFF)
            self.ma = (self.ma & _u(0xFFFF00FF)) | (byte << _u(8))
            return self.ma
        if self.form == "bitop3":
            # v_lshrrev_b32 (deg - 48), v_bitop3 (x & 0xFF00) | lwm
            return ((self.h1 >> _u(self.deg - 48)) & _u(0xFF00)) | self.lwm
        h = (self.h1 << _u(32)) | self.h0
        return (((h >> _u(self.deg - 8)) & _u(255)) << _u(8)) | self.lwm

    def step(self, new, old=None):
        """slide<K, TSH> (old given) or slide_in (the window still filling)."""
        o = self._lds((old << _u(8)) | self.lwo) if old is not None else np.zeros_like(self.h0)
        a1 = ((self.h1 << _u(8)) | (self.h0 >> _u(24))) & U32      # v_alignbit(h1, h0, 24)
        m = self._lds(self._mod_addr())
        self.h0 = ((((self.h0 << _u(8)) & U32) | new) ^ (o & U32) ^ (m & U32))
        self.h1 = a1 ^ (o >> _u(32)) ^ (m >> _u(32))


def _scan_segments(data, n, poly, form, mask, small, lo, hi):
    """scan_segment over every lane's segment [l * S, l * S + 64 + S) of `data`
    (zero-padded), counting the stream positions lo <= p < hi.  Returns the
    candidate flags per position and the lanes' (first, last, count)."""
    nl = max((n - 64 + S - 1) // S, 1)
    buf = np.zeros(nl * S + 64, np.uint64)
    buf[:n] = data[:n]
    voff = np.arange(nl, dtype=np.int64) * S
    # rel r of lane l is the window ending at p = voff + 65 + r
    p0 = voff + 65
    rlo = np.clip(lo - p0, 0, S)
    rhi = np.clip(np.minimum(hi, n + 1) - p0, 0, S)
    L = Lanes(nl, poly, form)
    for b in range(64):  # warm_unit
        L.step(buf[voff + b])
    first = np.full(nl, NONE, np.int64)
    last = np.full(nl, NONE, np.int64)
    count = np.zeros(nl, np.int64)
    cand = np.zeros(n + 2, bool)
    mask_u = _u(mask)
    for rb in range(0, S, G):  # scan_unit, one group
        hk = []
        accw = np.full(nl, 0xFFFF, np.uint64)
        for j in range(G):
            r = rb + j
            L.step(buf[voff + 64 + r], buf[voff + r])
            hk.append(L.h0.copy())
            t = (L.h0 & mask_u) if small else L.h0
            accw = np.minimum(accw & _u(0xFFFF), t & _u(0xFFFF))  # v_min_u16 accw, t, accw
        flagged = (accw & _u(0xFFFF)) == 0                         # acc == 0 && lv
        if not flagged.any():
            continue
        # record_group on the flagged lanes
        anyv = np.zeros(nl, np.uint64)
        for h in hk:
            anyv |= h
        hb = np.zeros(nl, np.int64)
        for j, h in enumerate(hk):
            hb |= ((h & mask_u) == 0).astype(np.int64) << j
        hb = np.where((anyv & mask_u) == 0, (1 << G) - 1, hb)
        glo = np.clip(rlo - rb, 0, G)
        ghi = np.clip(rhi - rb, 0, G)
        hb &= ((1 << ghi) - 1) & ~((1 << glo) - 1)
        hb = np.where(flagged, hb, 0)
        for l in np.nonzero(hb)[0]:
            bits = int(hb[l])
            count[l] += bin(bits).count("1")
            last[l] = rb + bits.bit_length() - 1
            if first[l] == NONE:
                first[l] = rb + (bits & -bits).bit_length() - 1
            for j in range(G):
                if bits >> j & 1:
                    cand[p0[l] + rb + j] = True
    return cand, (first, last, count), p0


def _zone_hashes(data, s_, z, n, poly, form):
    """h0 of the 64 min-zone positions z .. z + 63 (zone_wave_fast: 64 slide_in
    steps over 0 ++ b[z-64, z-1) ++ b[z, z+k), its last 64 bytes)."""
    x = np.zeros(128, np.uint64)
    x[1:64] = data[z - 64:z - 1]
    m = min(64, n - z)
    x[64:64 + m] = data[z:z + m]
    L = Lanes(64, poly, form)
    k = np.arange(64, dtype=np.int64)
    for i in range(64):
        L.step(x[k + i])
    return L.h0


def _model_cuts(data, params, poly, form):
    mn, avg, mx = params
    mask = avg - 1
    small = mask < 0xFFFF
    n = len(data)
    d64 = data.astype(np.uint64)
    # two passes whose counted ranges meet in the middle of a group
    mid = (n // 2) | 5
    c1, s1, p0 = _scan_segments(d64, n, poly, form, mask, small, 65, mid)
    c2, s2, _ = _scan_segments(d64, n, poly, form, mask, small, mid, n + 1)
    for cand, (first, last, count) in ((c1, s1), (c2, s2)):
        for l in range(len(p0)):  # the lanes' summaries are their candidates'
            seg = np.nonzero(cand[p0[l]:p0[l] + S])[0]
            assert count[l] == len(seg)
            if len(seg):
                assert (first[l], last[l]) == (seg[0], seg[-1])
            else:
                assert first[l] == NONE and last[l] == NONE
    assert not c1[mid:].any() and not c2[:mid].any()
    cand = c1 | c2
    cuts, s = [], 0
    while s < n:
        if n - s < mn:
            cuts.append(n)
            break
        z = s + mn
        cut = None
        zh = _zone_hashes(d64, s, z, n, poly, form)
        for k in range(64):
            pos = z + k
            if pos - s >= mx:
                cut = pos
            elif int(zh[k]) & mask == 0:
                cut = pos
            elif pos == n:
                cut = n
            if cut is not None:
                break
        if cut is None:
            end = min(s + mx, n)
            hits = np.nonzero(cand[z + 64:end])[0]
            cut = z + 64 + int(hits[0]) if len(hits) else end
        cuts.append(cut)
        s = cut
    return np.array(cuts, np.uint64)


@functools.lru_cache(maxsize=None)
def _data(name):
    rng = np.random.default_rng(7)
    rnd = rng.integers(0, 256, 768 * KiB + 77, dtype=np.uint8)
    if name == "random":
        return rnd
    if name == "zeros":
        return np.zeros(300 * KiB + 5, np.uint8)
    gap = rnd.copy()                        # zero runs shorter than either min
    gap[200 * KiB:200 * KiB + 7000] = 0
    gap[500 * KiB + 3:500 * KiB + 3 + 2500] = 0
    return gap


@pytest.mark.parametrize("poly,form", [(oracle.DEFAULT_POLY, "sdwa"), (GENERIC_POLY, "generic")])
@pytest.mark.parametrize("params", [NONSMALL, SMALL], ids=["mask_ffff", "small"])
@pytest.mark.parametrize("name", ["random", "zeros", "zero_run_below_min"])
def test_model_cuts_match_oracle(name, params, poly, form):
    data = _data(name)
    mn, avg, mx = params
    want = oracle.chunk_cuts(data, poly, mn, avg, mx)
    if name == "random":  # hit cuts, not max cuts alone
        sizes = np.diff(np.concatenate([[0], want.astype(np.int64)]))
        assert np.sum(sizes[:-1] < mx) >= 5
    got = _model_cuts(data, params, poly, form)
    assert np.array_equal(got, want), (name, got[:6], want[:6])


def test_address_forms_agree():
    """The one-instruction MOD address gives the two-instruction form's cuts."""
    data = _data("zero_run_below_min")
    a = _model_cuts(data, SMALL, oracle.DEFAULT_POLY, "sdwa")
    b = _model_cuts(data, SMALL, oracle.DEFAULT_POLY, "bitop3")
    assert np.array_equal(a, b)
    assert np.array_equal(a, oracle.chunk_cuts(data, oracle.DEFAULT_POLY, *SMALL))
