"""Every kind of captured sampler step on a real MI355X, through the samplers' public surface (tests/sampler_graph_cases.py): the keys
a sample puts into the engine's graph cache are the ones tests/golden/sampler_graph_keys.json holds -- recorded by
oracle/make_goldens_sampler_keys.py from the commit before the samplers' host code was folded (one capture gate, one buffer refresh,
one sample loop) -- a second sample on fresh inputs of the same shapes captures nothing, and its latents are torch.equal to the same
sampler class stepping launch by launch: every static buffer was refreshed, though a new tensor may sit at an old one's address.
torch's generator is left where the launch-by-launch run leaves it."""
import json
from pathlib import Path

import pytest
import torch

from tests import sampler_graph_cases as sg

GOLDEN = Path(__file__).resolve().parent / "golden" / "sampler_graph_keys.json"


def golden():
    return json.loads(GOLDEN.read_text())


def test_fixture_holds_exactly_the_scenarios():
    """no GPU: a scenario cannot drop out of the fixture or of the scenario file silently"""
    g = golden()
    assert set(g) == set(sg.SCENARIOS) and len(sg.SCENARIOS) == 10, sorted(set(g) ^ set(sg.SCENARIOS))
    assert all(keys and all(isinstance(k, str) for k in keys) for keys in g.values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sg.SCENARIOS))
def test_keys_are_the_parents_and_a_second_sample_replays(device, name):
    m = sg.model(device)
    first, second, got = sg.two_passes(name, m, device)
    print(f"[{name}] first pass put {[repr(k) for k in first]}, second {second}")
    assert [repr(k) for k in first] == golden()[name]
    assert second == []
    assert any(isinstance(k, tuple) and k and k[0] == first[-1][0] for k in m._engine._graphs), "the captured step never ran"
    want = sg.reference_pass(name, m, device)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.isfinite(a).all() and torch.equal(a, b), (i, (a - b).abs().max().item())
