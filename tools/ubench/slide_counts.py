"""VALU and DS instructions per byte of every slide_bench case, from the
disassembly of its instantiation, and the kernel's VGPR count.
usage: python tools/ubench/slide_counts.py [slide_bench.s]
(without an argument it compiles tools/ubench/slide_bench.hip for gfx950,
device code only, into a temporary file).

Per kernel: the straight-line blocks that hold a group of slides with its
prefilter (at least 8 ds_read_b64 and a v_min*), two lookups per byte and
chain; warm-up and rare-path blocks hold no v_min* and are left out.
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = {(105, 116, 16, 1, 1): "V0", (105, 116, 16, 1, 0): "V0r0", (105, 216, 16, 1, 1): "T1",
         (205, 116, 16, 1, 1): "A", (205, 16, 16, 1, 1): "A16", (105, 16, 16, 1, 1): "V16",
         (205, 1016, 16, 1, 1): "A16m", (105, 1016, 16, 1, 1): "V16m", (105, 116, 12, 1, 1): "W12",
         (105, 116, 12, 2, 1): "W12x2", (205, 116, 12, 2, 1): "A12x2"}


def disassembly():
    if len(sys.argv) > 1:
        return open(sys.argv[1]).read()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "slide_bench.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17",
                               "--offload-arch=gfx950", "-Wno-unused-function",
                               "--cuda-device-only", "-S", "-o", out,
                               os.path.join(HERE, "slide_bench.hip")])
        return open(out).read()


def main():
    text = disassembly()
    vgprs = dict(re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text))
    print(f"{'case':6s} {'VALU/byte':>9s} {'DS/byte':>8s} {'slow VALU/byte':>15s} {'VGPRs':>6s}"
          "   (slow: v_perm, v_alignbit, v_min3, v_pk_min, sdwa, SGPR operands)")
    for m in re.finditer(r"^(_Z10slide_kernILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])EEv\w+):.*?\n(.*?)^\.Lfunc_end",
                         text, re.S | re.M):
        sym, key, body = m[1], tuple(int(m[i]) for i in range(2, 7)), m[7]
        blocks = re.split(r"^\.LBB\S+:.*$|s_cbranch\S+.*$", body, flags=re.M)
        hot = [b for b in blocks if b.count("ds_read_b64") >= 8 and re.search(r"\bv_(pk_)?min", b)]
        ins = [l.strip() for b in hot for l in b.splitlines() if re.match(r"\s+(v_|ds_)", l)]
        valu = [l for l in ins if l.startswith("v_")]
        ds = [l for l in ins if l.startswith("ds_")]
        slow = [l for l in valu if re.match(r"v_(perm|alignbit|min3|pk_min)", l) or "sdwa" in l
                or re.search(r"\bs\d+\b|\bs\[", l)]
        nbytes = len([l for l in ds if l.startswith("ds_read_b64")]) / 2.0
        print(f"{NAMES.get(key, str(key)):6s} {len(valu) / nbytes:9.2f} {len(ds) / nbytes:8.2f} "
              f"{len(slow) / nbytes:15.2f} {vgprs.get(sym, '?'):>6s}")


if __name__ == "__main__":
    main()
