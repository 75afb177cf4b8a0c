"""What seer_attn_fwd and seer_attn_bwd refuse, and with which code, before anything is launched: no GPU needed.

The host checks of the three attention units share csrc/attn_common.h (attn_check_addressing, the launch choice of
seer_attn40_launch); this file pins the codes they return.  The table was taken from the build of the commit BEFORE those checks
moved (the expected codes were run against that library first), so it states what callers have always seen.

Every case starts from one descriptor per entry point that is valid -- and that is therefore never passed to the library, it would
launch -- and changes one thing about it, which gets the call refused ahead of any launch.  Pointers are the integer 16.
"""
import ctypes

import pytest

EINVAL, ENOSYS = -22, -38
P = 16


@pytest.fixture(scope="module")
def lib():
    from seervideoldm_amd import _lib
    from seervideoldm_amd.build import build_library
    build_library()
    return _lib.load()


def _fwd(**change):
    """the valid forward descriptor ([2 x 8 heads, 256, 40] self-attention on token-major rows of 320), with `change` applied.
    F / Fq / H / W describe 16 frames of 8 x 8 tokens: window_ws = 4 alone (16 frames of one 4 x 4 window = 256 positions) is valid too"""
    from seervideoldm_amd import _lib
    d = _lib.AttnDesc()
    d.Q = d.K = d.V = d.O = P
    d.q_bs = d.k_bs = d.v_bs = d.o_bs = 256 * 320
    d.q_ss = d.k_ss = d.v_ss = d.o_ss = 320
    d.batch, d.heads, d.head_dim, d.Sq, d.Sk = 2, 8, 40, 256, 256
    d.scale = 40 ** -0.5
    d.F, d.Fq, d.H, d.W = 16, 16, 8, 8
    for k, v in change.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    return d


def _bwd(fwd=None, **change):
    """the valid backward descriptor around _fwd(lse = P, **fwd), with `change` applied to the backward's own fields"""
    from seervideoldm_amd import _lib
    d = _lib.AttnBwdDesc()
    d.fwd = _fwd(**{"lse": P, **(fwd or {})})
    d.dO = d.dQ = d.dK = d.dV = d.delta = P
    d.do_bs = d.dq_bs = d.dk_bs = d.dv_bs = 256 * 320
    d.do_ss = d.dq_ss = d.dk_ss = d.dv_ss = 320
    for k, v in change.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    return d


FWD_CASES = [
    ("Q NULL", dict(Q=None), EINVAL),
    ("K NULL", dict(K=None), EINVAL),
    ("V NULL", dict(V=None), EINVAL),
    ("O NULL", dict(O=None), EINVAL),
    ("batch 0", dict(batch=0), EINVAL),
    ("q_ss 12", dict(q_ss=12), EINVAL),
    ("o_ss 6", dict(o_ss=6), EINVAL),
    ("k_bs 12", dict(k_bs=12), EINVAL),
    ("q_hs -8", dict(q_hs=-8), EINVAL),
    ("q_hs 4", dict(q_hs=4), EINVAL),
    ("window_ws 5", dict(window_ws=5), EINVAL),
    ("window_ws 4, H 6", dict(window_ws=4, H=6), EINVAL),
    ("window_ws 4, Sq != Fq * 16", dict(window_ws=4, Fq=8), EINVAL),
    ("window_ws 4, Fq 0", dict(window_ws=4, Fq=0), EINVAL),
    ("variant -1", dict(variant=-1), EINVAL),
    ("variant 4", dict(variant=4), EINVAL),
    ("variant 8", dict(variant=8), EINVAL),
    ("variant 2 at head_dim 80", dict(variant=2, head_dim=80), EINVAL),
    ("causal_offset -1", dict(causal_offset=-1), EINVAL),
    ("causal, Sq + causal_offset > Sk", dict(causal=1, causal_offset=1), EINVAL),
    ("F16 with lse", dict(flags=2, lse=P), EINVAL),
    ("F16 with variant 2", dict(flags=2, variant=2), EINVAL),
    ("head_dim 64", dict(head_dim=64), ENOSYS),
    # the two below pass seer_attn_fwd's own checks and are refused inside seer_attn40_launch
    ("d = 40 ring form on half a query block", dict(variant=7, Sq=128), EINVAL),                      # needs whole 256-query blocks
    ("d = 40, K byte offsets past 2^32", dict(variant=3, Sk=1 << 20, k_ss=4096), ENOSYS),
]

BWD_POINTERS = [("fwd", n) for n in ("Q", "K", "V", "O", "lse")] + [("bwd", n) for n in ("dO", "dQ", "dK", "dV", "delta")]

BWD_CASES = [
    *[(f"{n} NULL", dict(fwd={n: None}) if where == "fwd" else {n: None}, EINVAL) for where, n in BWD_POINTERS],
    ("q_hs set", dict(fwd=dict(q_hs=8)), ENOSYS),
    ("q prescaled", dict(fwd=dict(flags=1)), ENOSYS),
    ("dq_ss 6", dict(dq_ss=6), EINVAL),
    ("windowed, Fq != F", dict(fwd=dict(window_ws=4, Fq=8)), EINVAL),
    ("windowed, Sk != Sq", dict(fwd=dict(window_ws=4, Sk=128)), EINVAL),
    ("head_dim 64", dict(fwd=dict(head_dim=64)), ENOSYS),
]


def test_flag_values_match_the_binding():
    from seervideoldm_amd import _lib
    assert (_lib.SEER_ATTN_Q_PRESCALED, _lib.SEER_ATTN_F16) == (1, 2)
    assert len(BWD_POINTERS) == 10


def test_null_descriptors(lib):
    assert lib.seer_attn_fwd(None, None) == EINVAL
    assert lib.seer_attn_bwd(None, None) == EINVAL


@pytest.mark.parametrize("change,code", [c[1:] for c in FWD_CASES], ids=[c[0] for c in FWD_CASES])
def test_attn_fwd_refuses(lib, change, code):
    assert lib.seer_attn_fwd(ctypes.byref(_fwd(**change)), None) == code


@pytest.mark.parametrize("change,code", [c[1:] for c in BWD_CASES], ids=[c[0] for c in BWD_CASES])
def test_attn_bwd_refuses(lib, change, code):
    assert lib.seer_attn_bwd(ctypes.byref(_bwd(**change)), None) == code
