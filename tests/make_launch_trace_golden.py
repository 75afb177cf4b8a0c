"""Writes tests/golden/engine_launch_trace.json.gz: the launches of every walk of tests/launch_trace.py (the full-size engine on the
meta device, every form of the engine at the small 320-wide config, the trainer's forward_backward), as THIS checkout issues them:
    python -m tests.make_launch_trace_golden
Run on the commit whose launches are the reference -- the parent of a change that must not move a launch -- and carry the file over.
The project's own code only.  The commit's hash goes into the file's metadata."""
import gzip
import json
import subprocess
from pathlib import Path

from tests import launch_trace

ROOT = Path(__file__).resolve().parents[1]
OUT = Path(__file__).parent / "golden" / "engine_launch_trace.json.gz"


def main():
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(["git", "status", "--porcelain", "--", "seervideoldm_amd"], cwd=ROOT, capture_output=True, text=True,
                           check=True).stdout.strip()
    assert not dirty, f"the package differs from {commit}:\n{dirty}"
    walks, chains = launch_trace.record_all()
    doc = {"meta": {"commit": commit, "walks": len(walks), "calls": sum(len(v) for v in walks.values()), "max_rowchains": chains},
           "walks": walks}
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(OUT, OUT.stat().st_size, "bytes", doc["meta"])


if __name__ == "__main__":
    main()
