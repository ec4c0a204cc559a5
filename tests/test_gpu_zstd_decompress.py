"""Frames decompressed on the device (rcdc_zstd_decompress, rcdc_zstd_dx.hip):
decode_all of the read path (crates/core/src/backend/decrypt.rs:71-97).

Parity bar: libzstd (oracle/zstd_ref.py).  A frame the device decodes (status
0) gives exactly the bytes libzstd's streaming decoder gives; the frames it
refuses are the ones the frame checker (rcdc_zstd_check, itself pinned to
libzstd and, in three places, to the stricter RFC 8878) refuses.  Every call
here writes into a buffer pre-filled with a guard byte, the outputs at ragged
offsets, and asserts that no byte outside any [out_off, out_off + out_cap)
changed.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import zstd_ref as zr
from tests import zstd_frames as zf
from tests.test_gpu_zstd_check import KINDS, LENS, _check, _data, _device_frames, _layout

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decompress(ctx, frames, caps, seed=5):
    """(status, out_lens, outputs) of one call; asserts the guard bytes."""
    import torch
    from rustic_core_amd.compress import decompress_frames
    rng = np.random.default_rng(seed)
    farr, foffs = _layout(frames, 1)
    ooffs, o = [], 0
    for c in caps:
        o += int(rng.integers(1, 17))
        ooffs.append(o)
        o += int(c)
    total = o + 64
    out = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda:0")
    d_f = torch.from_numpy(farr).to("cuda:0")
    st, ln = decompress_frames(ctx, d_f.data_ptr(), foffs, [len(f) for f in frames], out.data_ptr(),
                               ooffs, caps)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    outside = np.ones(total, bool)
    for a, c in zip(ooffs, caps):
        outside[a:a + int(c)] = False
    assert (h[outside] == GUARD).all(), "a byte outside the output ranges changed"
    assert all(int(n) <= int(c) for n, c in zip(ln, caps))
    assert all(int(n) == 0 for s, n in zip(st, ln) if s != 0)
    return st, ln, [h[a:a + int(n)].tobytes() for a, n in zip(ooffs, ln)]


def _stats(ctx):
    from rustic_core_amd.compress import decompress_stats
    return decompress_stats(ctx)


def _compressed_blocks(frame):
    return sum(1 for t, size, _ in zr.blocks(frame) if t == 2 and size)


def _assert_decoded(ctx, frames, datas, caps=None):
    st, ln, outs = _decompress(ctx, frames, [len(d) for d in datas] if caps is None else caps)
    bad = [(i, int(st[i]), int(ln[i]), len(datas[i])) for i in range(len(datas))
           if st[i] != 0 or outs[i] != datas[i]]
    assert bad == [], f"(frame, status, out_len, expected length): {bad[:10]}"


# ---- this library's encoder and libzstd's -----------------------------------

@pytest.mark.parametrize("level", [0, 1, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_own_frames(gpu_ctx, kind, level):
    rng = np.random.default_rng(sum(kind.encode()) + level)
    datas = [_data(rng, n, kind) for n in LENS]
    frames = _device_frames(gpu_ctx, datas, level)
    _assert_decoded(gpu_ctx, frames, datas)
    s = _stats(gpu_ctx)
    # neither treeless literals nor repeat-mode tables: all in the parallel pass
    assert s["frames"] == len(frames) and s["blocks_in_order"] == 0 and s["groups"] == 1
    assert s["blocks_parallel"] == sum(_compressed_blocks(f) for f in frames)


@pytest.mark.parametrize("level", [-5, 1, 3, 9, 19])
def test_libzstd_frames(gpu_ctx, level):
    rng = np.random.default_rng(1000 + level)
    datas = [_data(rng, n, k) for k in KINDS for n in (1, 5000, 200001, 700000)]
    frames = [zr.compress(d, level) for d in datas]
    _assert_decoded(gpu_ctx, frames, datas)


@pytest.mark.parametrize("how", ["checksum", "no content size", "window log 10"])
def test_libzstd_advanced_frames(gpu_ctx, how):
    from rustic_core_amd.compress import frame_info
    rng = np.random.default_rng(77)
    datas = [_data(rng, n, k) for k in KINDS for n in (1, 5000, 200001)]
    kw = {"checksum": dict(checksum=True), "no content size": dict(content_size=False),
          "window log 10": dict(window_log=10)}[how]
    frames = [zr.compress_adv(d, 3, **kw) for d in datas]
    caps = None
    if how == "no content size":  # decoded into the bound the block headers give
        info = [frame_info(f) for f in frames]
        assert all(cs is None or len(d) == 0 for (cs, _, _), d in zip(info, datas))
        caps = [b for _, b, _ in info]
        assert all(c >= len(d) for c, d in zip(caps, datas))
    _assert_decoded(gpu_ctx, frames, datas, caps)
    if how == "checksum":  # a wrong checksum is malformed
        bad = [f[:-1] + bytes([f[-1] ^ 0x40]) for f in frames]
        st, _, _ = _decompress(gpu_ctx, bad, [len(d) for d in datas])
        assert st.tolist() == [2] * len(bad)


def test_treeless_literals_in_the_parallel_pass(gpu_ctx):
    """libzstd's level-3 frame of 700000 bytes of text has treeless literals
    sections (most of its blocks) and no repeat-mode table: the parallel pass
    rebuilds each table from the earlier block's tree description and the
    frame never goes to the in-order pass."""
    from tests import zstd_dissect as zd
    rng = np.random.default_rng(1003)
    d = _data(rng, 700000, "text")
    f = zr.compress(d, 3)
    blocks = zd.dissect(f).blocks
    treeless = sum(1 for b in blocks if b.type == 2 and b.literals.type == 3)
    repeat = sum(1 for b in blocks if b.type == 2 and b.sequences.modes is not None and
                 3 in ((b.sequences.modes >> 6) & 3, (b.sequences.modes >> 4) & 3,
                       (b.sequences.modes >> 2) & 3))
    assert treeless >= 1 and repeat == 0
    _assert_decoded(gpu_ctx, [f], [d])
    s = _stats(gpu_ctx)
    assert s["treeless_resolved"] == treeless and s["blocks_in_order"] == 0
    assert s["blocks_parallel"] == _compressed_blocks(f)


# ---- the hand-built case table ----------------------------------------------

def _libzstd(frame):
    try:
        return zr.decompress_stream(frame)
    except zr.ZstdError:
        return None


def case_caps(cases):
    """out_cap per case: what libzstd decodes, or the blob's / declared size."""
    from rustic_core_amd.compress import frame_info
    caps = []
    for c in cases:
        dec = _libzstd(c.frame)
        try:
            cs = frame_info(c.frame)[0] or 0
        except Exception:
            cs = 0
        caps.append(len(dec) if dec is not None else max(len(c.blob), cs if cs < 1 << 24 else 0))
    return caps


def judge_cases(cases, st, outs):
    """The cases the device got wrong: (name, expected, status)."""
    wrong = []
    for c, s, o in zip(cases, st, outs):
        s = int(s)
        if c.expect_status == 0:
            ok = s == 0 and o == c.blob
        elif c.expect_status == 2:
            ok = s == 2
        else:  # the blob differs from the frame's content: libzstd judges the frame
            dec = _libzstd(c.frame)
            ok = (s == 0 and o == dec) if dec is not None else s != 0
        if not ok:
            wrong.append((c.name, c.expect_status, s))
    return wrong


def run_cases(ctx, cases):
    st, _, outs = _decompress(ctx, [c.frame for c in cases], case_caps(cases))
    return judge_cases(cases, st, outs)


def test_case_table(gpu_ctx):
    cases = zf.CASES
    assert len(cases) == 306
    assert [sum(c.expect_status == k for c in cases) for k in (0, 1, 2)] == [160, 69, 77]
    assert sum(c.stricter is not None for c in cases) == 3
    names = {c.name for c in cases}
    assert "every compare path once" in names and all(n in names for n, *_ in zf.BLOCK_PARALLEL)
    # 67 of the 69 status-1 cases are frames libzstd decodes; the two it
    # refuses declare a content size one off
    refused = [c.name for c in cases if c.expect_status == 1 and _libzstd(c.frame) is None]
    assert sorted(refused) == ["hdr content size + 1", "hdr content size - 1"]
    assert run_cases(gpu_ctx, cases) == []
    assert run_cases(gpu_ctx, cases[::-1]) == []


def _tool(mode, **env):
    e = dict(os.environ, **env)
    e.pop("RCDC_ZSTD_DBG", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "zdx_cases.py"), mode], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_case_table_in_order_pass():
    """The same table with every frame's entropy decoded in order
    (RCDC_ZDX_BLOCKS=0 is read once per process: a fresh one)."""
    got = _tool("cases", RCDC_ZDX_BLOCKS="0")
    assert got["cases"] == len(zf.CASES) and got["wrong"] == []
    assert got["stats"]["blocks_parallel"] == 0 and got["stats"]["blocks_in_order"] > 0


def test_groups():
    """RCDC_ZDX_WS_MAX=1 MiB: 40 frames of mixed kinds and sizes run in groups
    of whole frames and decode equal."""
    got = _tool("groups", RCDC_ZDX_WS_MAX="1048576")
    assert got["frames"] == 40 and got["wrong"] == []
    assert got["stats"]["groups"] > 1


# ---- repeat offsets across blocks ---------------------------------------------

def _history_frame(first, lax=False, last_offset=47):
    """A raw block, a block that leaves the history (last_offset, 33, 20), and
    a block that opens with the sequences `first`; each block describes its
    own tables."""
    rng = np.random.default_rng(3)
    c = zf.Content(lax)
    blocks = [c.raw(zf._rb(rng, 64))]
    blocks.append(c.block(zf._rb(rng, 40), [(3, 4, 20 + 3), (2, 5, 33 + 3), (1, 6, last_offset + 3)]))
    blocks.append(c.block(zf._rb(rng, 40), first + [(2, 4, 2), (0, 4, 1), (1, 3, 3), (0, 5, 3)]))
    return zf.frame(blocks, len(c.out)), c.blob()


def test_repeat_history_across_blocks(gpu_ctx):
    frames, blobs = [], []
    for ofv in (1, 2, 3):
        for ll in (0, 2):
            f, b = _history_frame([(ll, 5, ofv)])
            assert zr.decompress_stream(f) == b
            frames.append(f)
            blobs.append(b)
    _assert_decoded(gpu_ctx, frames, blobs)
    s = _stats(gpu_ctx)
    assert s["blocks_in_order"] == 0 and s["blocks_parallel"] == 2 * len(frames)
    # the block before ends with offset 1: value 3 with no literals is 1 - 1 = 0
    f, b = _history_frame([(0, 5, 3)], lax=True, last_offset=1)
    st, _, _ = _decompress(gpu_ctx, [f], [len(b)])
    assert st.tolist() == [2]


# ---- matches -------------------------------------------------------------------

def _raw_seq_block(lits, seqs, regen):
    return (2, zf.lit_raw(lits) + zf.seq_section(seqs)[0], regen)


def test_matches(gpu_ctx):
    rng = np.random.default_rng(4)
    frames, blobs, names = [], [], []

    def add(name, blocks, c, **kw):
        f = zf.frame(blocks, len(c.out), **kw) if "wd" not in kw else zf.frame(blocks, **kw)
        assert zr.decompress_stream(f) == c.blob(), name
        frames.append(f)
        blobs.append(c.blob())
        names.append(name)

    c = zf.Content()
    add("offset 1, 120000 bytes", [c.raw(b"x" * 10), c.block(zf._rb(rng, 5), [(5, 120000, 1 + 3)])], c)
    c = zf.Content()
    add("offset < length", [c.raw(zf._rb(rng, 64)), c.block(zf._rb(rng, 12), [(10, 50, 7 + 3)])], c)
    c = zf.Content()
    add("offset < length, long", [c.raw(zf._rb(rng, 64)), c.block(zf._rb(rng, 12), [(10, 5000, 37 + 3)])], c)
    c = zf.Content()
    add("offset == length", [c.raw(zf._rb(rng, 64)), c.block(zf._rb(rng, 12), [(10, 50, 50 + 3)])], c)
    c = zf.Content()
    add("offset == length, long", [c.raw(zf._rb(rng, 640)), c.block(zf._rb(rng, 12), [(10, 500, 500 + 3)])], c)
    # the third block reaches back exactly to the frame's first byte
    c = zf.Content()
    lits = zf._rb(rng, 25)
    add("back to the first byte", [c.raw(zf._rb(rng, 1000)), c.rle(7, 500),
                                   c.block(lits, [(20, 30, 1520 + 3)])], c)
    blocks = [(0, c.blob()[:1000], 1000), (1, bytes([7]), 500)]
    before = zf.frame(blocks + [_raw_seq_block(lits, [(20, 30, 1521 + 3)], 55)], 1555)
    # a 1 KiB window (blocks of at most 1 KiB): an offset at it and just past it
    c = zf.Content()
    raws = [c.raw(zf._rb(rng, 1000)) for _ in range(3)]
    lits = zf._rb(rng, 15)
    add("offset at the window", raws + [c.block(lits, [(10, 20, 1024 + 3)])], c, fcs_bytes=0,
        wd=zf.window_desc(10))
    past = zf.frame(raws + [_raw_seq_block(lits, [(10, 20, 1025 + 3)], 35)], fcs_bytes=0,
                    wd=zf.window_desc(10))
    # a batch of 64 sequences, each match's source the match before it
    c = zf.Content()
    add("chain of 64", [c.raw(zf._rb(rng, 8)), c.block(b"", [(0, 8, 8 + 3)] * 64)], c)
    c = zf.Content()
    add("chain of 150 with literals", [c.raw(zf._rb(rng, 8)),
                                       c.block(zf._rb(rng, 155), [(1, 7, 8 + 3)] * 150)], c)
    c = zf.Content()
    add("chain of 64 long matches", [c.raw(zf._rb(rng, 100)), c.block(b"", [(0, 100, 100 + 3)] * 64)], c)
    st, ln, outs = _decompress(gpu_ctx, frames + [before, past],
                               [len(b) for b in blobs] + [1555, 3035])
    wrong = [n for n, s, o, b in zip(names, st, outs, blobs) if s != 0 or o != b]
    assert wrong == []
    assert st.tolist()[-2:] == [2, 2]


# ---- capacity --------------------------------------------------------------------

def test_capacity(gpu_ctx):
    from rustic_core_amd.compress import frame_info
    rng = np.random.default_rng(6)
    datas = [_data(rng, 300001, "text"), _data(rng, 5000, "random"), _data(rng, 200000, "zeros"),
             _data(rng, 140000, "csv")]
    for kw in (dict(), dict(content_size=False)):
        frames = [zr.compress_adv(d, 3, **kw) for d in datas] + \
            [zf.frame([(0, datas[1], len(datas[1]))], len(datas[1]))]
        want = datas + [datas[1]]
        st, ln, _ = _decompress(gpu_ctx, frames, [len(d) - 1 for d in want])
        assert st.tolist() == [1] * len(frames) and ln.tolist() == [0] * len(frames)
        st, ln, outs = _decompress(gpu_ctx, frames, [len(d) + 1 + 1000 * i for i, d in enumerate(want)])
        assert st.tolist() == [0] * len(frames) and outs == want
    # without a content size: decoded into the bound of the block headers
    frames = [zr.compress_adv(d, 3, content_size=False) for d in datas]
    caps = [frame_info(f)[1] for f in frames]
    assert all(frame_info(f)[0] is None for f in frames)
    st, ln, outs = _decompress(gpu_ctx, frames, caps)
    assert st.tolist() == [0] * len(frames) and outs == datas
    assert _decompress(gpu_ctx, [], [])[0].tolist() == []


# ---- corrupted frames --------------------------------------------------------------

@pytest.mark.parametrize("source", ["device", "libzstd"])
def test_corrupted_frames(gpu_ctx, source):
    """The corruptions of test_gpu_zstd_check.test_corrupted_frames_agree_with_libzstd
    (5 blobs x (40 single-bit flips + 1 truncation)).  Soundness: status 0
    implies libzstd's streaming decoder gives exactly the device's bytes.
    Agreement: for a frame libzstd decodes to bytes L, status 0 <=> the
    checker accepts (frame, L)."""
    rng = np.random.default_rng(11 if source == "device" else 12)
    base = [_data(rng, n, k) for k, n in [("text", 200000), ("csv", 150000), ("binary", 140000),
                                         ("mixed", 400000), ("periodic", 90000)]]
    good = _device_frames(gpu_ctx, base) if source == "device" else [zr.compress(d, 3) for d in base]
    frames, datas = [], []
    for f, d in zip(good, base):
        for _ in range(40):
            g = bytearray(f)
            i = int(rng.integers(5, len(g)))
            g[i] ^= 1 << int(rng.integers(0, 8))
            frames.append(bytes(g))
            datas.append(d)
        frames.append(f[:len(f) - int(rng.integers(1, 8))])  # truncated
        datas.append(d)
    dec = [_libzstd(f) for f in frames]
    caps = [len(L) if L is not None else len(d) + 64 for L, d in zip(dec, datas)]
    st, ln, outs = _decompress(gpu_ctx, frames, caps)
    unsound = [i for i, s in enumerate(st) if s == 0 and outs[i] != dec[i]]
    assert unsound == []
    idx = [i for i, L in enumerate(dec) if L is not None]
    ck = _check(gpu_ctx, [frames[i] for i in idx], [dec[i] for i in idx])
    differ = [(i, int(st[i]), int(c)) for i, c in zip(idx, ck) if (st[i] == 0) != (c == 0)]
    assert differ == []
    # as in that test, a corruption survives when the frame still decodes to the
    # blob: fewer than half do (a flipped literal decodes, to other bytes)
    survive = sum(1 for i, s in enumerate(st) if s == 0 and outs[i] == datas[i])
    assert survive < len(frames) // 2


def test_decode_all(gpu_ctx):
    """compress.decode_all: one frame through HBM; the reference's error."""
    from rustic_core_amd.compress import DECODE_MESSAGE, decode_all
    from rustic_core_amd.errors import ErrorKind, RusticError
    rng = np.random.default_rng(8)
    d = _data(rng, 150000, "text")
    assert decode_all(zr.compress(d, 3)) == d
    assert decode_all(zr.compress_adv(d, 3, content_size=False)) == d
    assert decode_all(zr.compress(b"", 3)) == b""
    f = bytearray(zr.compress(d, 3))
    f[len(f) // 2] ^= 0x55
    for bad in (bytes(f), b"not a frame", zr.compress(d, 3)[:-2]):
        with pytest.raises(RusticError) as e:
            decode_all(bad)
        assert e.value.kind == ErrorKind.Internal and e.value.message == DECODE_MESSAGE
