"""The ported slide (one-instruction MOD address, rcdc_slide.h TSH >= 200)
in the walk and the scan, against the CPU oracle at small shapes.

Streams of 4 MiB and 4 MiB + 77 bytes at min 32 KiB / avg 64 KiB / max 512 KiB
(mask 0xFFFF: the non-SMALL prefilter, a hit about every 64 KiB, so hits fall
in every lane and every phase of the 16-byte groups), the same streams at avg
8 KiB (the masked SMALL prefilter; min is 8 KiB there, the chunker refuses
min > avg), and one 16 MiB stream at rustic's defaults (the degree-53 kernels
the port changes).  Each set runs walked (pieces of 1 MiB), on the scan path,
and walked in pipelined runs.
"""
import functools

import numpy as np
import pytest

from oracle import oracle

KiB = 1 << 10
MiB = 1 << 20
NONSMALL = (32 * KiB, 64 * KiB, 512 * KiB)
SMALL = (8 * KiB, 8 * KiB, 512 * KiB)
DEFAULT = (oracle.DEFAULT_MIN, oracle.DEFAULT_AVG, oracle.DEFAULT_MAX)
SETS = {"nonsmall": (NONSMALL, (4 * MiB, 4 * MiB + 77)),
        "small": (SMALL, (4 * MiB, 4 * MiB + 77)),
        "default": (DEFAULT, (16 * MiB,))}


@functools.lru_cache(maxsize=None)
def _streams(name):
    _, lens = SETS[name]
    bufs = tuple(np.random.default_rng(900 + i).integers(0, 256, n, dtype=np.uint8)
                 for i, n in enumerate(lens))
    for b in bufs:
        b.setflags(write=False)
    return bufs


@functools.lru_cache(maxsize=None)
def _expected(name):
    mn, avg, mx = SETS[name][0]
    return tuple(oracle.chunk_cuts(b, oracle.DEFAULT_POLY, mn, avg, mx) for b in _streams(name))


def _hit_cuts(name):
    """Cuts of stream 0 that are neither max cuts nor the stream's end."""
    mx = SETS[name][0][2]
    cuts = _expected(name)[0].astype(np.int64)
    sizes = np.diff(np.concatenate([[0], cuts]))
    return int(np.sum((sizes < mx) & (cuts < len(_streams(name)[0]))))


def test_small_shapes_have_hit_cuts():
    """The 4 MiB cases cannot pass on max cuts alone."""
    assert _hit_cuts("nonsmall") >= 32
    assert _hit_cuts("small") >= 32


def _plan(name):
    import torch
    from rustic_core_amd.chunker import Context
    from rustic_core_amd.device import DevicePlan, pack_offsets
    mn, avg, mx = SETS[name][0]
    bufs = _streams(name)
    lens = [len(b) for b in bufs]
    offs, alen = pack_offsets(lens)
    host = np.zeros(alen, np.uint8)
    for o, b in zip(offs, bufs):
        host[int(o):int(o) + len(b)] = b
    dev = torch.from_numpy(host).to("cuda:0")
    ctx = Context.get(oracle.DEFAULT_POLY, mn, avg, mx, device=0)
    return DevicePlan(ctx, offs, lens, alen), dev


def _check(name, got):
    for i, (g, e) in enumerate(zip(got, _expected(name))):
        assert np.array_equal(g, e), (name, i, len(g), len(e))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("path", ["walk", "scan", "pipelined"])
def test_slide_paths_match_oracle(gpu_ctx, monkeypatch, name, path):
    import torch
    monkeypatch.setenv("RCDC_WALK_PIECE", "0" if path == "scan" else str(1 * MiB))
    monkeypatch.setenv("RCDC_WALK_MIN_PIECES", "1")
    plan, dev = _plan(name)
    info = plan.info()
    if path == "scan":
        assert info["walk_pieces"] == 0, info
    else:
        assert info["walk_pieces"] > 0, info
    if path == "pipelined":
        plan.set_pipeline(True)
        s = torch.cuda.Stream()
        for _ in range(3):
            plan.run(dev.data_ptr(), s.cuda_stream)
    else:
        plan.run(dev.data_ptr())
    got = plan.results()
    if path == "pipelined":
        plan.set_pipeline(False)
    plan.close()
    _check(name, got)
