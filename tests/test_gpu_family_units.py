"""The host units of the kernel families on one context (rcdc_aead.cpp,
rcdc_zstd_host.cpp, rcdc_place.cpp; their state in rcdc_ctx.h): a context's
whole life with every family used, page-locked buffers that grow between
calls, the cached key, and two families at once.

Checkers, as in each family's own tests: oracle/crypto_ref.c for sealed bytes
and pack files, libzstd for frames, byte compares for the rest."""
import threading

import numpy as np
import pytest

from oracle import oracle, zstd_ref

pytestmark = pytest.mark.gpu

BLK = 128 << 10


def _new_ctx():
    from rustic_core_amd.chunker import Context
    return Context(oracle.DEFAULT_POLY, oracle.DEFAULT_MIN, oracle.DEFAULT_AVG, oracle.DEFAULT_MAX,
                   device=0)


def _destroy(ctx):
    from rustic_core_amd import _lib
    _lib.lib().rcdc_ctx_destroy(ctx._h)
    ctx._h = None


def _dev(host):
    import torch
    return torch.from_numpy(np.ascontiguousarray(host)).to("cuda:0")


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _arena(datas, align=16):
    offs, o = [], 0
    for d in datas:
        offs.append(o)
        o = (o + len(d) + align - 1) // align * align
    a = np.zeros(o + 64, np.uint8)
    for off, d in zip(offs, datas):
        a[off:off + len(d)] = np.frombuffer(d, np.uint8)
    return a, offs


def _seal(ctx, key, datas, nonces):
    """The sealed blobs, and the device buffer that holds them at `offs`."""
    import torch
    from rustic_core_amd.crypto import make_refs, sealed_layout
    arena, offs = _arena(datas)
    lens = [len(d) for d in datas]
    oo, olen = sealed_layout(lens)
    d_in = _dev(arena)
    d_out = torch.zeros(olen + 64, dtype=torch.uint8, device="cuda:0")
    key.seal_blobs(d_in.data_ptr(), make_refs(offs, lens, oo, b"".join(nonces)), d_out.data_ptr(),
                   ctx=ctx)
    out = d_out.cpu().numpy()
    return [out[int(a):int(a) + n + 32].tobytes() for a, n in zip(oo, lens)], d_out, oo


def _open(ctx, key, d_sealed, offs, lens):
    import torch
    from rustic_core_amd.crypto import make_refs
    outs = [i * ((max(lens) + 15) // 16 * 16) for i in range(len(lens))]
    d_out = torch.zeros(outs[-1] + max(lens) + 64, dtype=torch.uint8, device="cuda:0")
    st = key.open_blobs(d_sealed.data_ptr(), make_refs(offs, lens, outs), d_out.data_ptr(), ctx=ctx)
    out = d_out.cpu().numpy()
    return st, [out[a:a + n - 32].tobytes() for a, n in zip(outs, lens)]


def _compress(ctx, datas):
    """The frames of `datas`, and the device buffer and layout they are in."""
    import torch
    from rustic_core_amd.compress import compress_blobs, frame_layout, make_refs
    arena, offs = _arena(datas)
    lens = [len(d) for d in datas]
    fo, ftot = frame_layout(lens)
    d_in = _dev(arena)
    d_fr = torch.zeros(ftot + 64, dtype=torch.uint8, device="cuda:0")
    fl = compress_blobs(ctx, d_in.data_ptr(), make_refs(offs, lens, fo), d_fr.data_ptr())
    fh = d_fr.cpu().numpy()
    frames = [fh[int(a):int(a) + int(n)].tobytes() for a, n in zip(fo, fl)]
    return frames, d_fr, fo, fl, d_in, offs


def _every_family(ctx, rng):
    import torch
    from rustic_core_amd.compress import check_frames, decompress_frames
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.pack import build_packs, make_blobs, pack_layout, place_blobs
    key = Key(_rand(rng, 64))
    # seal and open 2 blobs
    datas = [_rand(rng, 1000), _rand(rng, 70001)]
    nonces = [_rand(rng, 16) for _ in datas]
    sealed, d_sealed, s_offs = _seal(ctx, key, datas, nonces)
    assert sealed == [oracle.seal(key._key, nc, d) for nc, d in zip(nonces, datas)]
    st, plain = _open(ctx, key, d_sealed, s_offs, [len(s) for s in sealed])
    assert not st.any() and plain == datas
    # one pack of the 2 blobs, sealed by the call, then from the sealed pair
    ids = [_rand(rng, 32) for _ in datas]
    hn = _rand(rng, 16)
    want, index = oracle.pack_file(key._key, [(0, d, i, nc, 0) for d, i, nc in zip(datas, ids, nonces)], hn)
    arena, offs = _arena(datas)
    d_in = _dev(arena)
    for raw in (False, True):
        blobs = make_blobs(s_offs if raw else offs, [len(s) for s in sealed] if raw else
                           [len(d) for d in datas], np.frombuffer(b"".join(ids), np.uint8),
                           np.frombuffer(b"".join(nonces), np.uint8))
        packs, total = pack_layout(blobs, [(0, 2)], np.frombuffer(hn, np.uint8), raw=raw)
        d_pack = torch.zeros(total + 64, dtype=torch.uint8, device="cuda:0")
        boffs = build_packs(ctx, key._key, (d_sealed if raw else d_in).data_ptr(), blobs, packs,
                            d_pack.data_ptr(), total, raw=raw)
        assert d_pack.cpu().numpy()[:total].tobytes() == want, raw
        assert [int(v) for v in boffs] == [o for o, _ in index]
        assert int(packs[0]["size"]) == len(want)
    # compress a 0-byte and a (128 KiB + 1)-byte blob, check, decompress
    text = (b"the quick brown fox " * 7000)[:BLK + 1]
    zd = [b"", text]
    frames, d_fr, fo, fl, d_zin, z_offs = _compress(ctx, zd)
    assert [zstd_ref.decompress(f) for f in frames] == zd
    assert list(check_frames(ctx, d_fr.data_ptr(), fo, fl, d_zin.data_ptr(), z_offs,
                             [len(d) for d in zd])) == [0, 0]
    d_dec = torch.full((2 * (BLK + 64),), 0xEE, dtype=torch.uint8, device="cuda:0")
    st, olens = decompress_frames(ctx, d_fr.data_ptr(), fo, fl, d_dec.data_ptr(), [0, BLK + 64],
                                  [64, BLK + 1])
    assert list(st) == [0, 0] and list(olens) == [0, BLK + 1]
    assert d_dec.cpu().numpy()[BLK + 64:2 * BLK + 65].tobytes() == text
    # place the 2 decoded blobs, zero blobs skipped
    d_file = torch.full((BLK + 100,), 0x77, dtype=torch.uint8, device="cuda:0")
    zero = place_blobs(ctx, [d_dec.data_ptr()], [2 * (BLK + 64)],
                       [(0, 0, 0, 0, 1), (BLK + 64, BLK + 1, 0, 1, 1)], [(5, 0), (9, 0)],
                       [d_file.data_ptr()], [BLK + 100], skip_zero=True)
    got = d_file.cpu().numpy()
    assert list(zero) == [1, 0] and got[9:BLK + 10].tobytes() == text
    assert (got[:9] == 0x77).all() and (got[BLK + 10:] == 0x77).all()


def test_context_lifetime(rcdc_lib, gpu_ctx):
    """Create, use every family once, destroy: three times over.  Then the
    contexts whose lazily made streams and events differ: one no family used,
    one only place used."""
    import torch
    from rustic_core_amd.pack import place_blobs
    rng = np.random.default_rng(0xFA41)
    for _ in range(3):
        ctx = _new_ctx()
        _every_family(ctx, rng)
        _destroy(ctx)
    _destroy(_new_ctx())
    ctx = _new_ctx()
    src = _dev(np.arange(5000, dtype=np.uint32).view(np.uint8))
    dst = torch.zeros(20000, dtype=torch.uint8, device="cuda:0")
    zero = place_blobs(ctx, [src.data_ptr()], [20000], [(0, 20000, 0, 0, 1)], [(0, 0)],
                       [dst.data_ptr()], [20000])
    assert list(zero) == [0] and torch.equal(src, dst)
    _destroy(ctx)
    torch.cuda.synchronize()


def test_page_locked_buffers_regrow(rcdc_lib, gpu_ctx):
    """On one context the upload buffer of the seals and the buffer of the
    place calls grow and are used again below their size: 1 blob, 512 blobs of
    16 bytes (512 x 96 B of descriptors pass the first buffer's 4 KiB or so),
    1 blob; 1 destination, 4096 (32 KiB of addresses), 1."""
    import torch
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.pack import place_blobs
    rng = np.random.default_rng(0xFA42)
    ctx = _new_ctx()
    key = Key(_rand(rng, 64))
    for n, size in ((1, 300), (512, 16), (1, 300)):
        datas = [_rand(rng, size) for _ in range(n)]
        nonces = [_rand(rng, 16) for _ in range(n)]
        sealed, _, _ = _seal(ctx, key, datas, nonces)
        assert sealed == [oracle.seal(key._key, nc, d) for nc, d in zip(nonces, datas)], n
    blob = np.frombuffer(_rand(rng, 1000), np.uint8).copy()
    src = _dev(blob)
    for nd in (1, 4096, 1):
        dst = torch.zeros(nd * 1024, dtype=torch.uint8, device="cuda:0")
        zero = place_blobs(ctx, [src.data_ptr()], [1000], [(0, 1000, 0, 0, nd)],
                           [(1024 * d + (d & 7), 0) for d in range(nd)], [dst.data_ptr()], [nd * 1024])
        want = np.zeros(nd * 1024, np.uint8)
        for d in range(nd):
            want[1024 * d + (d & 7):1024 * d + (d & 7) + 1000] = blob
        assert list(zero) == [0] and np.array_equal(dst.cpu().numpy(), want), nd
    _destroy(ctx)


def test_key_cache(rcdc_lib, gpu_ctx):
    """Key A, then B, then A on one context: each seal under its own key."""
    from rustic_core_amd.crypto import Key
    rng = np.random.default_rng(0xFA43)
    ctx = _new_ctx()
    a, b = Key(_rand(rng, 64)), Key(_rand(rng, 64))
    datas = [_rand(rng, 100), _rand(rng, 5000)]
    nonces = [_rand(rng, 16) for _ in datas]
    for key in (a, b, a):
        sealed, d_sealed, offs = _seal(ctx, key, datas, nonces)
        assert sealed == [oracle.seal(key._key, nc, d) for nc, d in zip(nonces, datas)]
    # opened with the other key, the last seal's blobs fail their MAC
    st, _ = _open(ctx, b, d_sealed, offs, [len(s) for s in sealed])
    assert list(st) == [1, 1]
    st, plain = _open(ctx, a, d_sealed, offs, [len(s) for s in sealed])
    assert not st.any() and plain == datas
    _destroy(ctx)


def test_two_families_at_once(rcdc_lib, gpu_ctx):
    """Two threads on one context, 8 iterations each: one compresses a fixed
    batch of 4 blobs, one seals a fixed batch of 4; every result equals the
    single-threaded one (the families' locks and scratch are separate)."""
    from rustic_core_amd.crypto import Key
    rng = np.random.default_rng(0xFA44)
    ctx = _new_ctx()
    key = Key(_rand(rng, 64))
    zd = [(b"abcdefgh" * 40000)[:n] for n in (0, 1, BLK, BLK + 1)]
    sd = [_rand(rng, n) for n in (16, 1000, 65537, 200000)]
    nonces = [_rand(rng, 16) for _ in sd]
    want_frames = _compress(ctx, zd)[0]
    want_sealed = _seal(ctx, key, sd, nonces)[0]
    assert [zstd_ref.decompress(f) for f in want_frames] == zd
    assert want_sealed == [oracle.seal(key._key, nc, d) for nc, d in zip(nonces, sd)]
    bad = []

    def run(what):
        try:
            for i in range(8):
                got = _compress(ctx, zd)[0] if what == "zstd" else _seal(ctx, key, sd, nonces)[0]
                if got != (want_frames if what == "zstd" else want_sealed):
                    bad.append((what, i))
        except Exception as e:  # (a thread's exception would otherwise be lost)
            bad.append((what, repr(e)))

    threads = [threading.Thread(target=run, args=(w,)) for w in ("zstd", "aead")]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad
    _destroy(ctx)
