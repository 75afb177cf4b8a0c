"""Records tests/golden/gemm_units_parent.json from the PARENT of a change to how the GEMM tile kernel is built or dispatched.

    SEER_HIP_LIB=PARENT/seervideoldm_amd/lib/libseer_hip.so python -m oracle.make_goldens_gemm_units [--asm PARENT/seervideoldm_amd/lib/obj]
                                                                                                      [--run] [-o OUT.json]

The library is named through SEER_HIP_LIB, never the one of this tree.  Three parts; a part that is not asked for is kept from OUT:
  plan_256  (always; host only) the five words of seer_gemm_plan for a plain 256 x 256 x 256 descriptor, per tile code 0 .. 24
  kernels   (--asm) the kernel symbols of seer_gemm_kernel and of the split-K reduce kernels in the device assembly the build
            keeps under lib/obj
  cases     (--run, on an MI355X) per case of tests/gemm_units_cases.py, the SHA-256 of what the library leaves in the outputs
Recorded results only; tests/test_gemm_units_host.py and tests/test_gpu_gemm_units.py compare the tree against them."""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from seervideoldm_amd import _lib  # noqa: E402
from tests import gemm_units_cases as guc  # noqa: E402

OUT = ROOT / "tests" / "golden" / "gemm_units_parent.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", type=Path)
    ap.add_argument("--run", action="store_true")
    ap.add_argument("-o", "--out", type=Path, default=OUT)
    args = ap.parse_args()
    if "SEER_HIP_LIB" not in os.environ:
        sys.exit("name the parent's library through SEER_HIP_LIB")
    lib = _lib.load()
    src = args.out if args.out.exists() else OUT
    g = json.loads(src.read_text()) if src.exists() else {}
    g["plan_256"] = {str(t): guc.plan_256(lib, t) for t in range(25)}
    if args.asm:
        g["kernels"] = sorted(k for f in sorted(args.asm.glob("gemm*gfx950.s")) for k in guc.KERNEL.findall(f.read_text()))
    if args.run:
        import torch
        dev = torch.device("cuda:0")
        g["cases"] = {}
        for case in guc.cases():
            launch = guc.Launch(case, dev)
            assert launch.plan(lib) == guc.expected_plan(case), (case["id"], launch.plan(lib))
            g["cases"][case["id"]] = launch.run(lib)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(g, indent=0, sort_keys=True) + "\n")
    print(f"{args.out}: {len(g.get('kernels', []))} kernels, {len(g.get('cases', {}))} cases")


if __name__ == "__main__":
    main()
