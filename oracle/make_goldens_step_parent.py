"""Records what a built libseer_hip.so computes for the cases of tests/step_cases.py -> tests/golden/step_parent.npz.

    SEER_HIP_LIB=PATH/libseer_hip.so python -m oracle.make_goldens_step_parent [-o OUT.npz]

The fixture pins the bits of the sampler-step kernels (csrc/sampler_step.hip): tests/test_gpu_step_parent.py compares the library
under test against it, every form of a case against the one recorded result.  It is recorded on the GPU from the PARENT of a
change to those kernels -- a library built from a checkout of that commit, named by SEER_HIP_LIB -- never from the code under
test, which is why the variable has to be set.  The Python side (ops.py) is the tree's own, so the parent library must be of the
tree's ABI: a change that renames an entry point or moves its arguments (ABI 27 folded the sampler step's twins) cannot be
recorded across, and the fixture in the tree stays as it was recorded.

What every form of a case shares is taken from the case's first form; the forms are also compared among themselves here, and a
parent whose forms disagree is reported and not recorded."""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

OUT = ROOT / "tests" / "golden" / "step_parent.npz"


def record(out_path: Path) -> int:
    import torch
    from seervideoldm_amd import _lib, ops
    from tests import step_cases as sc
    device = torch.device("cuda")
    print(f"recording from {_lib.lib_path()}")
    save, bad = {}, []
    for name in sc.CASES:
        first = None
        for form in sc.forms(name):
            shared, own = sc.run(name, form, ops, device)
            torch.cuda.synchronize()
            if first is None:
                first = shared
                save.update(sc.keys(name, form, shared, own))
            else:
                save.update(sc.keys(name, form, {}, own))
                bad += [f"{name}: {form} != {sc.forms(name)[0]} in {k}" for k in first
                        if not np.array_equal(first[k], shared[k])]
    if bad:
        raise SystemExit("the forms of this library disagree:\n" + "\n".join(bad))
    np.savez_compressed(out_path, **save)
    return len(save)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-o", "--out", type=Path, default=OUT)
    a = ap.parse_args(argv)
    if not os.environ.get("SEER_HIP_LIB"):
        raise SystemExit("SEER_HIP_LIB is not set: the fixture is recorded from the parent commit's library, not the tree's")
    n = record(a.out)
    print(f"{a.out}: {n} arrays, {a.out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
