"""pack.parse_header on packs the device built (rcdc_pack_build): the header,
opened on the device (Key.decrypt_data), parses back to the index entries the
build returned -- the inverse of the HeaderEntry layout
(repofile/packfile.rs:88-124, PackHeader::from_binary :228-242).
"""
import numpy as np
import pytest

from tests.test_gpu_pack import _build

pytestmark = pytest.mark.gpu


def test_parse_header_of_device_packs(gpu_ctx):
    """Three packs of ragged data / tree blobs, some with compressed entries:
    every parsed entry equals what went in, the offsets are the ones
    rcdc_pack_build reported, and header_size is the u32 at the pack's end
    less the 32 bytes of sealing."""
    from rustic_core_amd.crypto import Key
    from rustic_core_amd.pack import header_size, parse_header
    rng = np.random.default_rng(0x4EAD)
    key = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    lens = [0, 1, 15, 16, 17, 33, 1000, 4095, 65537, 3, 20000, 5, 64, 31]
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    specs = [(int(rng.integers(0, 2)), rng.integers(0, 256, 32, dtype=np.uint8),
              rng.integers(0, 256, 16, dtype=np.uint8).tobytes(),
              int(rng.integers(1, 1 << 20)) if i % 3 == 2 else 0) for i in range(len(lens))]
    groups = [(0, 5), (5, 6), (11, 3)]
    hn = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in groups]
    files, packs, offsets, _, _ = _build(key, datas, specs, groups, hn)
    k = Key(key)
    for (b0, n), f in zip(groups, files):
        hlen = int.from_bytes(f[-4:], "little")
        got = parse_header(k.decrypt_data(f[-4 - hlen:-4]))
        want = [(specs[i][0], int(offsets[i]), lens[i] + 32, specs[i][3], specs[i][1].tobytes())
                for i in range(b0, b0 + n)]
        assert [tuple(e) for e in got] == want
        assert header_size(got) == hlen - 32
