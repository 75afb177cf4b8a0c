"""Records the graph-cache keys of every captured sampler step -> tests/golden/sampler_graph_keys.json.

    python -m oracle.make_goldens_sampler_keys [-o OUT.json]

Run on the GPU from a checkout of the PARENT of a change to the samplers' host code (seervideoldm_amd/{ddim,plms,slots}.py,
step_graph.py), with tests/sampler_graph_cases.py and this file copied beside it -- never from the code under test.  For each scenario
of sampler_graph_cases.py the fixture holds the repr of every key handed to the engine's graph_put, in order, over a sample and a second
sample on fresh inputs; tests/test_gpu_sampler_graphs.py holds the tree's samplers to it.  A parent whose second pass captures
again, or whose captured latents differ from its own launch-by-launch ones, is reported and not recorded."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

OUT = ROOT / "tests" / "golden" / "sampler_graph_keys.json"


def record(out_path: Path) -> int:
    import torch
    from tests import sampler_graph_cases as sg
    device = torch.device("cuda:0")
    m = sg.model(device)
    save, bad = {}, []
    for name in sg.SCENARIOS:
        first, second, got = sg.two_passes(name, m, device)
        want = sg.reference_pass(name, m, device)
        if second:
            bad.append(f"{name}: the second pass put {second}")
        if len(got) != len(want) or not all(torch.equal(a, b) for a, b in zip(got, want)):
            bad.append(f"{name}: captured != launch by launch")
        save[name] = [repr(k) for k in first]
        print(name, save[name])
    if bad:
        raise SystemExit("this checkout does not pass its own scenarios:\n" + "\n".join(bad))
    out_path.write_text(json.dumps(save, indent=1) + "\n")
    return len(save)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-o", "--out", type=Path, default=OUT)
    a = ap.parse_args(argv)
    n = record(a.out)
    print(f"{a.out}: {n} scenarios, {a.out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
