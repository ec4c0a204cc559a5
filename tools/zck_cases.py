"""The conformance table of tests/zstd_frames.py through rcdc_zstd_check, one
call, statuses as one JSON line: {"names": [...], "expect": [...],
"statuses": [...]}.  RCDC_CHECK_BLOCKS is read once per process, so
tests/test_gpu_zstd_check.py starts this in a fresh process with
RCDC_CHECK_BLOCKS=0 to hold the in-order pass alone to the table; it also
serves to look at a build by hand (RCDC_LIB).

  python tools/zck_cases.py [block-parallel]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import zstd_frames as zf  # noqa: E402
from tests.test_gpu_zstd_check import _check  # noqa: E402


def main():
    from oracle import oracle
    from rustic_core_amd.chunker import Context
    ctx = Context.get(oracle.DEFAULT_POLY, oracle.DEFAULT_MIN, oracle.DEFAULT_AVG,
                      oracle.DEFAULT_MAX, device=0)
    if len(sys.argv) > 1 and sys.argv[1] == "block-parallel":
        cases = [zf.Case(*c, None) for c in zf.BLOCK_PARALLEL]
    else:
        cases = zf.CASES
    st = _check(ctx, [c.frame for c in cases], [c.blob for c in cases])
    print(json.dumps({"names": [c.name for c in cases], "expect": [c.expect_status for c in cases],
                      "statuses": [int(s) for s in st]}), flush=True)


if __name__ == "__main__":
    main()
