"""The conformance table of tests/zstd_frames.py through rcdc_zstd_decompress
in one process, the wrong cases and the pass counters as one JSON line.
RCDC_ZDX_BLOCKS and RCDC_ZDX_WS_MAX are read once per process, so
tests/test_gpu_zstd_decompress.py starts this in a fresh process with them
set; it also serves to look at a build by hand (RCDC_LIB).

  python tools/zdx_cases.py [cases | reversed | groups]

cases / reversed: {"cases": n, "wrong": [[name, expected, status], ...], "stats": {...}}
groups: 40 frames of mixed kinds and sizes (this library's and libzstd's),
        {"frames": 40, "wrong": [indices], "stats": {...}}
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import zstd_frames as zf  # noqa: E402
from tests import test_gpu_zstd_decompress as t  # noqa: E402


def main():
    from oracle import oracle, zstd_ref as zr
    from rustic_core_amd.chunker import Context
    from rustic_core_amd.compress import decompress_stats
    ctx = Context.get(oracle.DEFAULT_POLY, oracle.DEFAULT_MIN, oracle.DEFAULT_AVG,
                      oracle.DEFAULT_MAX, device=0)
    mode = sys.argv[1] if len(sys.argv) > 1 else "cases"
    if mode == "groups":
        rng = np.random.default_rng(40)
        sizes = [1, 300, 5000, 70000, 131073, 200001, 400000, 700000]
        datas = [t._data(rng, sizes[i % len(sizes)], t.KINDS[i % len(t.KINDS)]) for i in range(40)]
        frames = [zr.compress(d, 3) for d in datas[:20]] + t._device_frames(ctx, datas[20:])
        st, _, outs = t._decompress(ctx, frames, [len(d) for d in datas])
        wrong = [i for i in range(40) if st[i] != 0 or outs[i] != datas[i]]
        print(json.dumps({"frames": len(frames), "wrong": wrong, "stats": decompress_stats(ctx)}),
              flush=True)
        return
    cases = zf.CASES[::-1] if mode == "reversed" else zf.CASES
    wrong = t.run_cases(ctx, cases)
    print(json.dumps({"cases": len(cases), "wrong": wrong, "stats": decompress_stats(ctx)}), flush=True)


if __name__ == "__main__":
    main()
