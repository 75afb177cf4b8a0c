"""csrc/sampler_step.hip against tests/golden/step_parent.npz, bit for bit: what the commit before the kernels were folded into one
body per idea computed for the cases of tests/step_cases.py (recorded by oracle/make_goldens_step_parent.py from that commit's
library on an MI355X).  Where several forms of a step must agree -- host index, device counter, seeded fed the matching
seer_philox_normal tensor, slot, x_prev aliasing x -- the fixture holds ONE result and every form is held to it.  Outputs start
as NaN and are compared as int32 words, so an element a kernel must not write is part of the comparison.

The one behaviour the fold changed is tested last, on the tree's library alone: a device counter below zero in
seer_cfg_ddim_step_dev / seer_cfg_plms_step_dev moves the counter and state words as before and writes no element."""
from pathlib import Path

import numpy as np
import pytest
import torch

from seervideoldm_amd import ops
from tests import step_cases as sc

GOLDEN = Path(__file__).resolve().parent / "golden" / "step_parent.npz"
_golden = {}


def golden():
    if not _golden:
        with np.load(GOLDEN) as z:
            _golden.update({k: z[k] for k in z.files})
    return _golden


def test_fixture_holds_exactly_the_generators_cases():
    """no GPU: a case cannot drop out of the fixture or of the generator silently, nor a form that has words of its own"""
    names = {k.split("/")[0] for k in golden()}
    assert names == set(sc.CASES), (sorted(names - set(sc.CASES)), sorted(set(sc.CASES) - names))
    for k in golden():
        parts = k.split("/")
        assert len(parts) == 2 or parts[1] in sc.forms(parts[0]), k
    assert GOLDEN.stat().st_size < 300 * 1024


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.CASES))
def test_every_form_gives_the_parents_bits(device, name):
    g = golden()
    for form in sc.forms(name):
        shared, own = sc.run(name, form, ops, device)
        got = sc.keys(name, form, shared, own)
        want_keys = {k for k in g if k.startswith(name + "/") and (k.count("/") == 1 or k.startswith(f"{name}/{form}/"))}
        assert set(got) == want_keys, (form, sorted(set(got) ^ want_keys))
        for k, v in got.items():
            diff = np.flatnonzero(v != g[k])
            assert diff.size == 0, f"{k} ({form}): {diff.size} of {v.size} words differ, first at {diff[0]}: " \
                                   f"{int(v[diff[0]]):#x} != {int(g[k][diff[0]]):#x}"


# ---- a device counter below zero: the words move, no element is written -------------------------------------------------------------
def _negative_inputs(device):
    b = 2
    rng = np.random.default_rng(7)
    eps = torch.from_numpy(sc._eps(rng, b, sc.COND_F)).to(device)
    x = torch.from_numpy(sc._latent(rng, b)).to(device)
    coef = torch.from_numpy(sc.coef_table(0.8)).to(device)
    step = torch.tensor([7, -1], dtype=torch.int32, device=device)
    return eps, x, coef, step


def _untouched(*tensors):
    return all(bool((t.cpu().view(torch.int32) == int(sc.NAN_BITS)).all()) for t in tensors)


@pytest.mark.gpu
@pytest.mark.parametrize("with_noise", [False, True])
def test_ddim_step_dev_at_a_negative_counter_writes_no_element(device, with_noise):
    eps, x, coef, step = _negative_inputs(device)
    noise = torch.ones_like(x) if with_noise else None
    x_prev, pred = sc._nan(x.shape, device), sc._nan(x.shape, device)
    ops.cfg_ddim_step_dev(eps, x, coef, step, cfg=True, scale=sc.SCALE, cond_f=sc.COND_F, x_prev=x_prev, pred_x0=pred, noise=noise)
    assert step.tolist() == [-2, -1]
    assert _untouched(x_prev, pred)


@pytest.mark.gpu
def test_plms_step_dev_at_a_negative_counter_writes_no_element(device):
    eps, x, coef, step = _negative_inputs(device)
    x_prev, pred, ring = sc._nan(x.shape, device), sc._nan(x.shape, device), sc._nan((3, *x.shape), device)
    ring_state = torch.tensor([5, 5, 1, 0], dtype=torch.int32, device=device)        # index -1 is odd: it reads (valid, newest) = (1, 0)
    ops.cfg_plms_step_dev(eps, x, coef, step, ring, ring_state, cfg=True, scale=sc.SCALE, cond_f=sc.COND_F, x_prev=x_prev, pred_x0=pred)
    assert step.tolist() == [-2, -1]
    assert ring_state.tolist() == [2, 1, 1, 0]           # the pair of parity (index - 1) = (min(valid + 1, 3), (newest + 1) % 3)
    assert _untouched(x_prev, pred, ring)
