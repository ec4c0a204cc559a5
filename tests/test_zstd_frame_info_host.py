"""CPU: rcdc_zstd_frame_info (compress.frame_info), the header walk the read
path sizes a frame's output with, against libzstd on the hand-built frames of
tests/zstd_frames.py and on libzstd's own frames.  No GPU."""
import ctypes

import numpy as np
import pytest

from oracle import zstd_ref as zr
from tests import zstd_frames as zf


def _walk(frame):
    """Blocks of the first frame, walked here: (type, size) per block.  zr.blocks
    reads single-segment frames without flags only; this one reads the
    others the table holds (window descriptors, checksums, dictionary-id
    fields) the same way."""
    fhd = frame[4]
    single, did = (fhd >> 5) & 1, (0, 1, 2, 4)[fhd & 3]
    fcs = (1 if single else 0, 2, 4, 8)[fhd >> 6]
    pos = 5 + (0 if single else 1) + did + fcs
    out = []
    while True:
        h = int.from_bytes(frame[pos:pos + 3], "little")
        out.append(((h >> 1) & 3, h >> 3))
        pos += 3 + (1 if (h >> 1) & 3 == 1 else h >> 3)
        if h & 1:
            return out


def _decodable(cases):
    for c in cases:
        try:
            yield c.name, c.frame, zr.decompress_stream(c.frame)
        except zr.ZstdError:
            continue


def _agrees(name, frame, decoded):
    from rustic_core_amd.compress import frame_info
    cs, bound, nb = frame_info(frame)
    assert cs == zr.content_size(frame), name
    assert bound >= len(decoded), name
    try:
        want = len(zr.blocks(frame))
    except zr.ZstdError:
        want = len(_walk(frame))
    assert nb == want, name
    # exact where no block is compressed
    if all(t != 2 for t, _ in _walk(frame)):
        assert bound == len(decoded), name


def test_case_table(rcdc_lib):
    """Every case libzstd's streaming decoder decodes.  One of them, "skippable
    frame first", does not begin with a zstd frame: the streaming decoder
    skips the skippable frame and decodes the one behind it, while
    zr.content_size answers 0 for the skippable frame and zr.blocks refuses
    it, so the three comparisons have no reference there.  frame_info
    describes the first frame and refuses that one, as the device does
    (status 2); that is asserted instead."""
    from rustic_core_amd.compress import frame_info
    from rustic_core_amd.errors import ErrorKind, RusticError
    seen = skipped = 0
    for name, frame, decoded in _decodable(zf.CASES):
        if frame[:4] != zf.MAGIC:
            assert name == "skippable frame first"
            with pytest.raises(RusticError) as e:
                frame_info(frame)
            assert e.value.kind == ErrorKind.InvalidInput
            skipped += 1
            continue
        _agrees(name, frame, decoded)
        seen += 1
    assert seen >= 160 and skipped == 1  # every status-0 case decodes, and most status-1 ones


@pytest.mark.parametrize("level", [1, 3, 19])
@pytest.mark.parametrize("with_size", [True, False])
def test_libzstd_frames(rcdc_lib, level, with_size):
    rng = np.random.default_rng(level)
    for n in (0, 1, 5000, 131072, 131073, 400001):
        d = (bytes(rng.integers(97, 101, n).astype(np.uint8)) + bytes(n))[:n]
        f = zr.compress_adv(d, level, content_size=with_size)
        assert zr.decompress_stream(f) == d
        _agrees((level, with_size, n), f, d)
        if not with_size and n:
            from rustic_core_amd.compress import frame_info
            assert frame_info(f)[0] is None


def test_refusals(rcdc_lib):
    from rustic_core_amd.compress import frame_info
    from rustic_core_amd.errors import ErrorKind, RusticError
    d = bytes(range(256)) * 40
    f = zr.compress(d, 3)
    raw = zf.frame([(0, d[:100], 100), (0, d[100:300], 200)], 300)
    assert frame_info(raw) == (300, 300, 2)
    hdr_end = 5 + 2  # magic, descriptor, a 2-byte content size
    bad = [b"", f[:3], f[:5], f[:hdr_end - 1],       # the frame header cut off
           f[:hdr_end], f[:hdr_end + 2],              # no room for a block header
           f[:len(f) - 1], raw[:-1],                  # the last block past the end
           raw[:len(raw) - 200 - 3 + 2],              # the second block's header cut off
           b"\x27" + f[1:],                           # another magic
           f[:4] + bytes([f[4] | 8]) + f[5:],         # the reserved bit
           zf.frame([(3, b"", 0)], 0)]                # the reserved block type
    for b in bad:
        with pytest.raises(RusticError) as e:
            frame_info(b)
        assert e.value.kind == ErrorKind.InvalidInput, b[:16]


def test_ref_struct_size(rcdc_lib):
    from rustic_core_amd.compress import ZSTD_DEC_REF, ZstdDecRef
    assert ctypes.sizeof(ZstdDecRef) == 32 and ZSTD_DEC_REF.itemsize == 32
    assert [f[0] for f in ZstdDecRef._fields_] == list(ZSTD_DEC_REF.names)
