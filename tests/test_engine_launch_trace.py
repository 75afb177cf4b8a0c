"""The engine and the trainer issue the launches they issued before their block walk and their launch-form plan became single
(unet.block_sequence, unet._LaunchPlan): every walk of tests/launch_trace.py is recorded again and compared, call by call, with
tests/golden/engine_launch_trace.json.gz -- recorded by tests/make_launch_trace_golden.py on the commit named in the file's metadata,
the parent of that change.  CPU only; the layout-invariant full-size walks ask the built library's host-side fold query."""
import gzip
import json
from pathlib import Path

import pytest

from tests import launch_trace

GOLDEN = Path(__file__).parent / "golden" / "engine_launch_trace.json.gz"


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN, "rb") as f:
        doc = json.loads(f.read().decode())
    assert len(doc["meta"]["commit"]) == 40 and doc["meta"]["walks"] == len(doc["walks"])
    return doc["walks"]


def _same(name, got, want):
    got = json.loads(json.dumps(got))           # (tuples -> lists, as the fixture went through JSON)
    if got == want:
        return
    i = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    lines = [f"{name}: {len(got)} calls against {len(want)} recorded; first difference at call {i}"]
    for k in range(max(i - 3, 0), i + 3):
        lines += [f"  [{k}] now      {got[k] if k < len(got) else '--'}", f"  [{k}] recorded {want[k] if k < len(want) else '--'}"]
    print("\n".join(lines))
    raise AssertionError(lines[0])


def _check(walks, golden, prefix):
    assert set(walks) == {k for k in golden if k.startswith(prefix)}
    for name, calls in walks.items():
        _same(name, calls, golden[name])


def test_full_size_walks_issue_the_recorded_launches(golden):
    walks, chains = launch_trace.full_size_walks()
    assert len(walks) == 32
    _check(walks, golden, "full/")
    # non-vacuity: the default walk of the 32x32 level moves with the batch and with the device, and row chains do run
    # (by the op names alone: the shapes differ with the batch anyway)
    d = lambda B, cus: [c[0] for c in walks[f"full/default/B{B}/cond0/H32/cus{cus}"]]
    assert d(1, 256) != d(2, 256) and d(1, 256) != d(1, 32)
    assert chains > 0 and "rowchain" in d(2, 256)
    assert all(len(v) > 400 for v in walks.values())


def test_small_config_walks_issue_the_recorded_launches(golden):
    walks = launch_trace.small_walks()
    _check(walks, golden, "small/")
    forms = {k.split("/", 2)[2] for k in walks}
    assert {"plain", "fold_ln=False", "freeu", "return_attn", "layout_invariant=on"} | {s + "=off" for s in launch_trace.SWITCHES} <= forms
    # every cached evaluation is a shorter walk than the storing one of its branch; 320 channels at every level: chains below level 0 too
    cached = [k for k in walks if k.endswith("/phase1")]
    assert len(cached) == 2 * (launch_trace.SMALL_CFG["layers_per_block"] + 1)
    for k in cached:
        assert 0 < len(walks[k]) < len(walks[k[:-1] + "0"]), k
    assert sum(c[0] == "rowchain" for c in walks["small/B1F2H16c0/plain"]) > 3
    assert not any(c[0] == "rowchain" for c in walks["small/B1F2H16c0/rowchain=off"])


def test_trainer_walks_issue_the_recorded_launches(golden):
    walks = launch_trace.trainer_walks()
    assert len(walks) == 3
    _check(walks, golden, "trainer/")
    assert all(any(c[0].endswith("_bwd") for c in v) for v in walks.values())      # forward and backward in one trace
