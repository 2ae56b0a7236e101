#!/usr/bin/env python3
"""Are the SIFT kernels of two builds the same device code?

  hipcc <FLAGS of tests/test_kernel_isa.py> colmap-pcd_amd/csrc/sift.hip -o a.s     (at each of the two commits)
  python tools/sift_isa_diff.py a.s b.s

Per pcd::k_sift_* kernel: the instruction stream between its label and .Lfunc_end (comment lines dropped, trailing
comments cut, .L label numbers normalised) and the vgpr / sgpr / LDS / scratch figures of the metadata.  Exit status 1
if any kernel differs or exists in one file only."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_kernel_isa import _kernels  # noqa: E402


def _stream(body):
    out = []
    for ln in body.split("\n"):
        ln = ln.split(";")[0].strip()
        if ln:
            out.append(re.sub(r"\.L\w+", ".L", ln))
    return out


def main(a, b):
    (ma, ba), (mb, bb) = _kernels(open(a).read()), _kernels(open(b).read())
    names = sorted(k for k in set(ma) | set(mb) if "k_sift_" in k)
    bad = 0
    for k in names:
        if k not in ma or k not in mb or k not in ba or k not in bb:
            print(f"ONLY IN ONE  {k}")
            bad += 1
            continue
        sa, sb = _stream(ba[k]), _stream(bb[k])
        same = sa == sb and ma[k] == mb[k]
        bad += not same
        print(f"{'same' if same else 'DIFFERENT':9}  {len(sa):6} instr  {ma[k]}  {k}")
        if ma[k] != mb[k]:
            print(f"           second file: {len(sb)} instr  {mb[k]}")
    print(f"{len(names)} kernels, {bad} different")
    return 1 if bad or not names else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
