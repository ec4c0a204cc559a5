"""rcdc_place_blobs (pack.place_blobs) on the device: decoded blobs scattered
to their file positions (commands/restore.rs:630-668), with the all-zero test
of SparseRestore::ByContent.  The expectation is numpy's, on the host.  Every
output is a view into a larger tensor with 64 guard bytes of 0xA5 on both
sides, which must not change; every source blob lies between 0xFF bytes."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 65535, 65536, 65537, (1 << 20) + 3]


class Layout:
    """Sources and outputs of one call: blobs laid into 0xFF-filled source
    buffers at chosen alignments, destinations into guarded outputs."""

    def __init__(self, n_ins=1, n_outs=1, fill=0x5A):
        self.ins = [[np.full(GUARD, 0xFF, np.uint8)] for _ in range(n_ins)]
        self.in_len = [GUARD] * n_ins
        self.out_len = [0] * n_outs
        self.blobs, self.dests, self.datas = [], [], []
        self.fill = fill

    def _at(self, pos, align):
        return pos + ((align - pos) & 15)

    def blob(self, data, src=0, in_align=0, outs=()):
        """outs: (dst, out_align) per destination."""
        data = np.asarray(data, np.uint8)
        o = self._at(self.in_len[src], in_align)
        self.ins[src].append(np.full(o - self.in_len[src], 0xFF, np.uint8))
        self.ins[src].append(data)
        self.ins[src].append(np.full(5, 0xFF, np.uint8))
        self.in_len[src] = o + len(data) + 5
        self.blobs.append((o, len(data), src, len(self.dests), len(outs)))
        for dst, oa in outs:
            p = self._at(self.out_len[dst] + 3, oa)
            self.dests.append((p, dst))
            self.out_len[dst] = p + len(data)
        self.datas.append(data)

    def run(self, gpu_ctx, skip_zero=False):
        """Places, checks guards and bytes against numpy; returns the flags."""
        import torch
        from rustic_core_amd.pack import place_blobs
        srcs = [torch.from_numpy(np.concatenate(p + [np.full(GUARD, 0xFF, np.uint8)])).to("cuda:0")
                for p in self.ins]
        bigs = []
        for n in self.out_len:
            b = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
            b[GUARD:GUARD + n] = self.fill
            bigs.append(b)
        outs = [b[GUARD:GUARD + n] for b, n in zip(bigs, self.out_len)]
        zero = place_blobs(gpu_ctx, [s.data_ptr() for s in srcs], [int(s.numel()) for s in srcs],
                           self.blobs, self.dests, [o.data_ptr() for o in outs], self.out_len,
                           skip_zero=skip_zero)
        torch.cuda.synchronize()
        want_zero = np.array([int(not d.any()) for d in self.datas], np.uint8)
        assert np.array_equal(zero, want_zero)
        exp = [np.full(n + 2 * GUARD, 0xA5, np.uint8) for n in self.out_len]
        for e, n in zip(exp, self.out_len):
            e[GUARD:GUARD + n] = self.fill
        for (o, n, src, d0, nd), data, z in zip(self.blobs, self.datas, want_zero):
            for p, dst in self.dests[d0:d0 + nd]:
                if not (skip_zero and z):
                    exp[dst][GUARD + p:GUARD + p + n] = data
        for b, e in zip(bigs, exp):
            got = b.cpu().numpy()
            bad = np.flatnonzero(got != e)
            assert bad.size == 0, (bad[:8] - GUARD, len(e) - 2 * GUARD)
        return zero


def test_lengths_and_alignments(gpu_ctx):
    rng = np.random.default_rng(7)
    L = Layout()
    for n in LENGTHS:
        L.blob(rng.integers(1, 256, n, dtype=np.uint8), 0, int(rng.integers(16)),
               [(0, int(rng.integers(16)))])
    for ia in range(16):
        for oa in range(16):
            L.blob(rng.integers(1, 256, 100, dtype=np.uint8), 0, ia, [(0, oa)])
    pairs = {(L.blobs[k][0] & 15, L.dests[L.blobs[k][3]][0] & 15)
             for k in range(len(LENGTHS), len(L.blobs))}
    assert len(pairs) == 256
    L.run(gpu_ctx)


def test_fan_out_two_sources(gpu_ctx):
    rng = np.random.default_rng(8)
    L = Layout(n_ins=2, n_outs=2)
    L.blob(rng.integers(0, 256, 70001, dtype=np.uint8), 1, 5, [(0, 3), (1, 9), (1, 0)])
    L.blob(rng.integers(0, 256, 300, dtype=np.uint8), 0, 11, [])      # only the zero test
    L.blob(np.zeros(40, np.uint8), 0, 2, [])
    L.blob(rng.integers(0, 256, 4097, dtype=np.uint8), 0, 7, [(1, 13), (0, 13)])
    assert list(L.run(gpu_ctx)) == [0, 0, 1, 0]


def _zero_cases(n):
    cases = [np.zeros(n, np.uint8)]
    for k in (0, n - 1, 65536, 65535):
        if k < n:
            d = np.zeros(n, np.uint8)
            d[k] = 1
            cases.append(d)
    return cases


@pytest.mark.parametrize("n", [200000, 3])
def test_zero_flags(gpu_ctx, n):
    L = Layout()
    for k, d in enumerate(_zero_cases(n)):
        # (a tile boundary is at blob offset 65536 whatever the alignment)
        L.blob(d, 0, (5 * k + 1) & 15, [(0, (3 * k) & 15)])
    L.blob(np.zeros(n, np.uint8), 0, 13, [(0, 6)])   # 0xFF on both sides, misaligned
    L.blob(np.zeros(0, np.uint8), 0, 9, [(0, 1)])    # the empty blob
    z = L.run(gpu_ctx)
    assert list(z) == [1] + [0] * (len(z) - 3) + [1, 1]


def _mixed(rng):
    L = Layout(n_outs=2)
    L.blob(np.zeros(70000, np.uint8), 0, 3, [(0, 5), (1, 2)])
    L.blob(rng.integers(1, 256, 70000, dtype=np.uint8), 0, 8, [(1, 7)])
    d = np.zeros(140000, np.uint8)
    d[139999] = 9   # the last tile alone is non-zero: the first ones are written too
    L.blob(d, 0, 1, [(0, 0), (0, 15)])
    L.blob(np.zeros(10, np.uint8), 0, 4, [(1, 1)])
    L.blob(np.zeros(0, np.uint8), 0, 4, [(1, 1)])
    L.blob(np.arange(33, dtype=np.uint8), 0, 15, [(0, 9)])
    return L


def test_skip_zero(gpu_ctx):
    """RCDC_PLACE_SKIP_ZERO: the destinations of all-zero blobs keep their
    0x5A, all others are written, the flags are the same."""
    a = _mixed(np.random.default_rng(9)).run(gpu_ctx, skip_zero=False)
    b = _mixed(np.random.default_rng(9)).run(gpu_ctx, skip_zero=True)
    assert list(a) == list(b) == [1, 0, 0, 1, 1, 0]


def test_windows(gpu_ctx, monkeypatch):
    """A tile list above the cap runs in windows: with SKIP_ZERO every tile of
    a blob is tested before any of it is written."""
    monkeypatch.setenv("RCDC_PLACE_TILES", "2")
    a = _mixed(np.random.default_rng(10)).run(gpu_ctx, skip_zero=True)
    b = _mixed(np.random.default_rng(10)).run(gpu_ctx, skip_zero=False)
    assert list(a) == list(b) == [1, 0, 0, 1, 1, 0]


def test_in_place_and_empty_call(gpu_ctx):
    import torch
    from rustic_core_amd.pack import place_blobs
    rng = np.random.default_rng(11)
    h = rng.integers(0, 256, 300000, dtype=np.uint8)
    t = torch.from_numpy(h).to("cuda:0")
    # [7, 100007) -> [150001, 250001) and [200, 211) -> [299989, 300000)
    z = place_blobs(gpu_ctx, [t.data_ptr()], [t.numel()], [(7, 100000, 0, 0, 1), (200, 11, 0, 1, 1)],
                    [(150001, 0), (299989, 0)], [t.data_ptr()], [t.numel()])
    torch.cuda.synchronize()
    exp = h.copy()
    exp[150001:250001] = h[7:100007]
    exp[299989:] = h[200:211]
    assert np.array_equal(t.cpu().numpy(), exp) and list(z) == [0, 0]
    # nblobs == 0
    assert len(place_blobs(gpu_ctx, [], [], [], [], [], [])) == 0
    assert len(place_blobs(gpu_ctx, [t.data_ptr()], [t.numel()], [], [], [t.data_ptr()],
                           [t.numel()], skip_zero=True)) == 0
    assert np.array_equal(t.cpu().numpy(), exp)


BIG = (1 << 64) - 1
INVALID = [
    # (name, blob overrides, dest overrides, call overrides, word of the message)
    ("src", dict(src=2), {}, {}, "src"),
    ("dst", {}, dict(dst=1), {}, "dst"),
    ("dest0+ndests", dict(dest0=1), {}, {}, "ndests_total"),
    ("dest0 overflow", dict(dest0=0xFFFFFFFF, ndests=2), {}, {}, "ndests_total"),
    ("in_off+len", dict(in_off=1000 - 99), {}, {}, "in_lens"),
    ("in_off overflow", dict(in_off=BIG - 10), {}, {}, "in_lens"),
    ("len overflow", dict(len=BIG), {}, {}, "in_lens"),
    ("out_off+len", {}, dict(out_off=2000 - 99), {}, "out_lens"),
    ("out_off overflow", {}, dict(out_off=BIG - 10), {}, "out_lens"),
    ("flags", {}, {}, dict(flags=2), "flags"),
    ("flags high", {}, {}, dict(flags=0x80000001), "flags"),
    ("null blobs", {}, {}, dict(blobs=None), "blobs"),
    ("null dests", {}, {}, dict(dests=None), "dests"),
    ("null d_ins", {}, {}, dict(d_ins=None), "d_ins"),
    ("null in_lens", {}, {}, dict(in_lens=None), "in_lens"),
    ("null d_outs", {}, {}, dict(d_outs=None), "d_outs"),
    ("null out_lens", {}, {}, dict(out_lens=None), "out_lens"),
    ("null ctx", {}, {}, dict(ctx=None), "ctx"),
]


@pytest.mark.parametrize("name,bo,do,co,word", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_input(gpu_ctx, name, bo, do, co, word):
    """Every case is refused on the host, before anything is launched: status
    2, the field named, source and output untouched."""
    import torch
    from rustic_core_amd import _lib
    from rustic_core_amd.pack import PLACE_BLOB, PLACE_DEST
    src = torch.full((1000,), 0x11, dtype=torch.uint8, device="cuda:0")
    out = torch.full((2000,), 0x22, dtype=torch.uint8, device="cuda:0")
    blobs = np.zeros(1, PLACE_BLOB)
    blobs[0] = (0, 100, 0, 0, 1, 0)
    dests = np.zeros(1, PLACE_DEST)
    dests[0] = (0, 0, 0)
    for k, v in bo.items():
        blobs[0][k] = v
    for k, v in do.items():
        dests[0][k] = v
    ins = (ctypes.c_void_p * 1)(src.data_ptr())
    outs = (ctypes.c_void_p * 1)(out.data_ptr())
    il, ol = np.array([1000], np.uint64), np.array([2000], np.uint64)
    zero = np.full(1, 7, np.uint8)
    a = dict(ctx=gpu_ctx.handle, d_ins=ctypes.cast(ins, ctypes.c_void_p), in_lens=il.ctypes.data,
             blobs=blobs.ctypes.data, dests=dests.ctypes.data,
             d_outs=ctypes.cast(outs, ctypes.c_void_p), out_lens=ol.ctypes.data, flags=0)
    a.update(co)
    st = _lib.lib().rcdc_place_blobs(a["ctx"], a["d_ins"], a["in_lens"], 1, a["blobs"], 1,
                                     a["dests"], 1, a["d_outs"], a["out_lens"], 1, a["flags"],
                                     zero.ctypes.data, None)
    assert st == 2
    assert word in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    assert bool((src == 0x11).all()) and bool((out == 0x22).all()) and zero[0] == 7
