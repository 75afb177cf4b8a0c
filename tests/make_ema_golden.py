"""Writes tests/golden/ema_litema.npz from the REFERENCE's own ldm/modules/ema.py (loaded by path; runs in the build container only,
where the reference tree is present):  python -m tests.make_ema_golden

LitEma is driven over a module of two parameters, `one` [1] and `big` [1000], whose values move between the updates as a training
run's would (a random walk; every snapshot lies on the fp16 grid, so the fixture stores the snapshots as fp16 without loss -- the
shadows are fp32 with full significands).  Three runs; data only:
    d0.9     decay 0.9,    100 updates   the warm-up min((1 + n) / (10 + n), decay) changes sides at n = 80
    d0.9999  decay 0.9999,  20 updates   the warm-up holds throughout
    nowarm   decay 0.9999,   5 updates   use_num_upates=False: one_minus_decay = 1 - decay from the first update
Per run R:  R_p0 fp16 [1001] the parameters LitEma was built on (its shadows start as their clone), R_p fp16 [U, 1001] the parameters
at every update, R_shadow fp32 [U, 1001] LitEma's buffers after every update, R_omd fp32 [U] the `one_minus_decay` of every update
(LitEma's expression on LitEma's own buffers; the script checks that it reproduces every recorded shadow bit for bit), R_decay,
R_warmup.  `sizes` = [1, 1000]: the flat layout."""
import importlib.util
from pathlib import Path

import numpy as np
import torch

OUT = Path(__file__).parent / "golden" / "ema_litema.npz"
SIZES = (1, 1000)
RUNS = (("d0.9", 0.9, True, 100), ("d0.9999", 0.9999, True, 20), ("nowarm", 0.9999, False, 5))


def _litema():
    from oracle.ref_import import REFERENCE_ROOT
    spec = importlib.util.spec_from_file_location("ref_ldm_ema", REFERENCE_ROOT / "ldm" / "modules" / "ema.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.LitEma


class _Model(torch.nn.Module):
    def __init__(self, flat):
        super().__init__()
        self.one = torch.nn.Parameter(flat[:1].clone())
        self.big = torch.nn.Parameter(flat[1:].clone())

    def flat(self):
        return torch.cat([self.one.detach(), self.big.detach()])


def _flat_shadow(ema):
    b = dict(ema.named_buffers())
    return torch.cat([b[ema.m_name2s_name["one"]], b[ema.m_name2s_name["big"]]]).clone()


def main():
    LitEma = _litema()
    arrays = {"sizes": np.asarray(SIZES, dtype=np.int64)}
    n = sum(SIZES)
    for seed, (name, decay, warmup, updates) in enumerate(RUNS):
        g = torch.Generator().manual_seed(100 + seed)
        grid = lambda t: t.to(torch.float16).float()
        p = p0 = grid(torch.randn((n,), generator=g))
        model = _Model(p)
        ema = LitEma(model, decay=decay, use_num_upates=warmup)
        ps, shadows, omds = [], [], []
        prev = _flat_shadow(ema)
        assert torch.equal(prev, p)
        for _ in range(updates):
            p = grid(p + 0.05 * torch.randn((n,), generator=g))
            with torch.no_grad():
                model.one.copy_(p[:1])
                model.big.copy_(p[1:])
            ema(model)
            d = ema.decay
            if ema.num_updates >= 0:
                d = min(ema.decay, (1 + ema.num_updates) / (10 + ema.num_updates))
            omd = 1.0 - d
            assert omd.dtype == torch.float32
            now = _flat_shadow(ema)
            assert torch.equal(now, prev - omd * (prev - p)), "the recorded one_minus_decay is not the one LitEma applied"
            ps.append(p.clone()); shadows.append(now); omds.append(omd.reshape(()))
            prev = now
        arrays[f"{name}_p0"] = p0.to(torch.float16).numpy()
        arrays[f"{name}_p"] = torch.stack(ps).to(torch.float16).numpy()
        arrays[f"{name}_shadow"] = torch.stack(shadows).numpy()
        arrays[f"{name}_omd"] = torch.stack(omds).numpy()
        arrays[f"{name}_decay"] = np.float64(decay)
        arrays[f"{name}_warmup"] = np.bool_(warmup)
        assert torch.equal(torch.stack(ps).to(torch.float16).float(), torch.stack(ps))
    np.savez_compressed(OUT, **arrays)
    print(OUT, OUT.stat().st_size, "bytes", len(arrays), "arrays")


if __name__ == "__main__":
    main()
