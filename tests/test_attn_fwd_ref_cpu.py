"""The constructions of tests/test_gpu_attn_fwd_matrix.py must be able to FAIL.  Here, without a GPU, the float64 emulation of
tests/attn_fwd_ref.py stands in for the kernel:

1. every Part 1 precondition holds on the reference alone (uniform_v / ramp_v assert them while they build: V and the expected O exact
   in the storage type, _exact_pre, "a level column moves after rounding when n is off by one"), and the unmutated emulation gives the
   expected O bit for bit;
2. the mutation table: every mutation of attn_fwd_ref.MUTATIONS applied to the emulation makes the Part 1 comparison report unequal
   bits, and the Part 2 worst-row error exceed 2x the unmutated emulation's, in every case where the mutation applies.  skip_p_round is
   the control: it must NOT fail (with Q = 0 every P is 1; on N(0, 1) inputs it only moves the error inside the 2x).

Where a mutation does not apply (emulate returns None): a single key (nothing to drop; one key counted twice is the same softmax), a
last key no query sees, Sk a whole number of tiles (no padded key to admit), no causal mask / no offset / one window.  An odd Sk
counts as ONE construction of two runs (pairs shifted by one): the key holding the zero of one run carries a w in the other.
The printed table is copied into profiles/attn_fwd_matrix.md."""
import pytest
import torch

from tests import attn_fwd_ref as R
from tests.test_gpu_train_matrix import _row_err

f16, bf16, f64 = torch.float16, torch.bfloat16, torch.float64
DEV = torch.device("cpu")
DTS = [pytest.param(bf16, id="bf16"), pytest.param(f16, id="f16")]
KINDS = ["generic", "a40_track", "a40_fast"]


def _bits_differ(o, want, dt):
    return not torch.equal(o.to(dt), want.expand(o.shape).to(dt))


def _part1_cases(d, dt):
    """(name, case, [(v4, want4), ...]): the runs of one construction"""
    out = []
    for i, (Sq, Sk) in enumerate(R.NONCAUSAL + R.RING):
        B, Hh = (2, 2, 1)[i % 3], (2, 1, 3)[i % 3]
        runs = [R.uniform_v(B, Hh, Sk, d, DEV, dt, seed=10 * i, shift=s) for s in ((0, 1) if Sk % 2 else (0,))]
        out.append((f"uniform {Sq}x{Sk}", R.plain(B, Hh, d, Sq, Sk), runs))
    for Sq, Sk, off in R.CAUSAL:
        out.append((f"ramp {Sq}x{Sk}+{off}", R.plain(2, 2, d, Sq, Sk, True, off), [R.ramp_v(2, 2, Sq, Sk, d, DEV, dt, off)]))
    for w in R.WINDOWS:
        case = R.window(1, 2, d, *w)
        out.append((f"ramp {case.name}", case, [R.ramp_v(1, 2, case.Sq, case.Sk, d, DEV, dt, case.off, case.windows)]))
    out.append(("ramp strided F12 L77", R.plain(77, 2, d, 12, 12, True, 0), [R.ramp_v(77, 2, 12, 12, d, DEV, dt)]))
    return out


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d", R.HEAD_DIMS)
def test_part1_preconditions_and_identity(d, dt):
    """the constructions build (their own asserts: exactness, _exact_pre, the level columns move) at every head_dim and storage type, and
    the unmutated emulation of every kernel kind reproduces the expected O bit for bit"""
    for name, case, runs in _part1_cases(d, dt):
        for v4, want4 in runs:
            q4 = torch.zeros((v4.shape[0], case.Hh, case.Sq, d), dtype=f64)
            for kind in (KINDS if d == 40 and dt == bf16 else KINDS[:2] if d == 40 else KINDS[:1]):
                r = R.emulate(q4, v4, v4, scale=d ** -0.5, dt=dt, kind=kind, causal=case.causal, off=case.off, windows=case.windows)
                assert not _bits_differ(r.o, want4, dt), f"{name} d{d} {kind}: the emulation does not give the expected O"
                n = r.n.to(f64)
                assert torch.equal(r.lse, torch.log2(n).expand(r.lse.shape)), f"{name}: lse of a uniform softmax is not log2(n)"


KIND_DT = [pytest.param(k, dt, id=f"{k}-{'f16' if dt == f16 else 'bf16'}") for k in KINDS for dt in (bf16, f16) if not (k == "a40_fast" and dt == f16)]


@pytest.mark.parametrize("kind,dt", KIND_DT)
def test_part1_mutations(kind, dt):
    """every applicable mutation changes at least one bit of O in every Part 1 construction; the control changes none (the fast path
    exists in bf16 only)"""
    d = 40
    table = {m: [0, 0] for m in R.MUTATIONS}
    for name, case, runs in _part1_cases(d, dt):
        for mut in R.MUTATIONS:
            seen, applies = False, False
            for v4, want4 in runs:
                q4 = torch.zeros((v4.shape[0], case.Hh, case.Sq, d), dtype=f64)
                r = R.emulate(q4, v4, v4, scale=d ** -0.5, dt=dt, kind=kind, causal=case.causal, off=case.off, windows=case.windows, mut=mut)
                if r is None:
                    continue
                applies = True
                seen |= _bits_differ(r.o, want4, dt)
            if not applies:
                continue
            table[mut][0] += 1
            table[mut][1] += seen
            if mut == "skip_p_round":
                assert not seen, f"{name}: the control changed O"
            else:
                assert seen, f"{name} {kind}: mutation {mut} leaves every bit of O in place"
    for mut, (n, hit) in table.items():
        print(f"attn_fwd_matrix mutations | part 1 | {kind} {'f16' if dt == f16 else 'bf16'} | {mut} | applicable {n} | seen {hit}")
        assert n > 0, f"{mut}: applicable nowhere"


def _part2_cases(d):
    cases = [R.plain((2, 2, 1)[i % 3], (2, 1, 3)[i % 3], d, Sq, Sk) for i, (Sq, Sk) in enumerate(R.NONCAUSAL)]
    cases += [R.plain(2, 2, d, Sq, Sk) for Sq, Sk in R.RING] if d == 40 else []
    cases += [R.plain(2, 2, d, Sq, Sk, True, off) for Sq, Sk, off in R.CAUSAL]
    cases += [R.window(1, 2, d, *w) for w in R.WINDOWS]
    cases += [R.plain(2, 2, d, *R.CROSS)]
    return cases


@pytest.mark.parametrize("kind,d,dt", [pytest.param(k, d, dt, id=f"{k}-d{d}-{'f16' if dt == f16 else 'bf16'}") for k, d in
                                       (("generic", 40), ("generic", 96), ("a40_track", 40), ("a40_fast", 40)) for dt in (bf16, f16)
                                       if not (k == "a40_fast" and dt == f16)])
def test_part2_mutations(kind, d, dt):
    """N(0, 1) inputs (the GPU file's own, same seeds), q x 1 and q x 3: every applicable mutation pushes the worst row past 2x the
    unmutated emulation's; without the P rounding the emulation stays inside it.  generic at 40 and 96: the denominator from the rounded
    and from the unrounded P"""
    table = {m: [0, 0, float("inf"), 0.0] for m in R.MUTATIONS}
    fails = []
    for case in _part2_cases(d):
        for qamp in (1.0, 3.0):
            q4, k4, v4 = R.to4(case, *R.inputs(case, dt, DEV, qamp))
            kw = dict(scale=d ** -0.5, dt=dt, kind=kind, causal=case.causal, off=case.off, windows=case.windows)
            base = R.emulate(q4, k4, v4, **kw)
            floor = R.row_floor(base.o_ref)
            e0 = _row_err(base.o, base.o_ref, floor)
            for mut in R.MUTATIONS:
                r = R.emulate(q4, k4, v4, mut=mut, **kw)
                if r is None:
                    continue
                e = _row_err(r.o, base.o_ref, floor)
                ratio = e / e0 if e0 > 0 else (float("inf") if e > 0 else 1.0)
                t = table[mut]
                t[0] += 1
                t[1] += ratio > 2
                t[2], t[3] = min(t[2], ratio), max(t[3], ratio)
                if (ratio > 2) == (mut == "skip_p_round"):
                    fails.append(f"{case.name} q x {qamp:g} {kind}: {mut} ratio {ratio:.3g}")
    for mut, (n, hit, lo, hi) in table.items():
        print(f"attn_fwd_matrix mutations | part 2 | {kind} d{d} {'f16' if dt == f16 else 'bf16'} | {mut} | applicable {n} | past 2x {hit} | "
              f"ratio {lo:.3g} .. {hi:.3g}")
    assert not fails, "\n".join(fails)


def test_kernel_kind_follows_the_dispatch():
    """the routing facts the emulation's roundings hang on (seer_attn_fwd, seer_attn40_launch)"""
    k = R.kernel_kind
    assert k(80, 0, bf16, 1024) == k(160, 0, f16, 77) == "generic"
    assert k(40, 0, bf16, 255) == "generic" and k(40, 0, bf16, 256) == "a40_fast" and k(40, 0, f16, 256) == "a40_track"
    assert k(40, 1, bf16, 1024) == k(40, 6, bf16, 1024) == k(40, 1, f16, 1024) == "generic"
    assert k(40, 2, bf16, 64) == k(40, 3, bf16, 64) == k(40, 7, bf16, 128) == "a40_fast"
    assert k(40, 5, bf16, 64) == k(40, 5, f16, 64) == k(40, 3, bf16, 64, lse=True) == "a40_track"
    assert k(40, 0, bf16, 1024, lse=True) == "generic" and k(40, 0, bf16, 1024, lse=True, prescaled=True) == "a40_track"
    assert R.l_rounded("generic", 40) and R.l_rounded("generic", 80) and not R.l_rounded("generic", 96) and R.l_rounded("a40_fast", 40)
