"""The host pieces the samplers' captured steps share, on plain CPU tensors: step_graph.refresh -- when a static buffer is refilled
from the tensor a caller brings -- and the two layout helpers next to ddim_sample, against the expressions they replaced."""
import gc
import weakref
from types import SimpleNamespace

import torch

from seervideoldm_amd import ddim, ops
from seervideoldm_amd.step_graph import refresh


def test_refresh_copies_when_the_source_is_new_or_was_written():
    kept, src, dst = {}, torch.arange(6.).reshape(2, 3), torch.zeros(2, 3)
    assert refresh(kept, "a", (src,), (dst,)) and torch.equal(dst, src)          # the first call copies
    dst.fill_(-1.)
    assert not refresh(kept, "a", (src,), (dst,)) and bool((dst == -1.).all())   # the same unchanged tensor: the buffer is left alone
    src.add_(1.)
    assert refresh(kept, "a", (src,), (dst,)) and torch.equal(dst, src)          # written in place: same address, another version
    dst.fill_(-1.)
    view = src.view_as(src)
    assert view is not src and view.data_ptr() == src.data_ptr() and view._version == src._version
    assert refresh(kept, "a", (view,), (dst,)) and torch.equal(dst, src)         # another tensor object over the same storage
    dst.fill_(-1.)
    assert not refresh(kept, "a", (view,), (dst,))
    assert refresh(kept, "b", (view,), (dst,))                                   # another name has a record of its own


def test_refresh_of_a_pair_copies_both_when_either_changed():
    kept = {}
    a, b = torch.ones(3), torch.full((2,), 2.)
    da, db = torch.zeros(3), torch.zeros(2)
    assert refresh(kept, "pair", (a, b), (da, db))
    for change in (lambda: a.mul_(3.), lambda: b.mul_(3.)):
        da.fill_(-1.), db.fill_(-1.)
        assert not refresh(kept, "pair", (a, b), (da, db)) and bool((da == -1.).all()) and bool((db == -1.).all())
        change()
        assert refresh(kept, "pair", (a, b), (da, db)) and torch.equal(da, a) and torch.equal(db, b)
    da.fill_(-1.), db.fill_(-1.)
    assert refresh(kept, "pair", (a, b.clone()), (da, db)) and torch.equal(da, a) and torch.equal(db, b)


def test_refresh_keeps_its_sources_alive():
    """the address of a freed tensor handed to the next sample's tensor must not look unchanged: the record holds the tensor"""
    kept, dst = {}, torch.zeros(4)
    src = torch.ones(4)
    ref = weakref.ref(src)
    refresh(kept, "a", (src,), (dst,))
    del src
    gc.collect()
    assert ref() is not None
    refresh(kept, "a", (torch.zeros(4),), (dst,))
    gc.collect()
    assert ref() is None                                  # and lets go of it when the next one comes


class _VAE:
    """shape-preserving and deterministic: decode is an affine map, encode hands back a posterior that adds one generator draw"""

    def __init__(self):
        self.draws = []

    def decode(self, z):
        return SimpleNamespace(sample=z * 0.5 + 0.125)

    def encode(self, frames):
        def sample(generator=None):
            noise = torch.randn(frames.shape, generator=generator)
            self.draws.append(noise)
            return frames + 0.25 * noise
        return SimpleNamespace(latent_dist=SimpleNamespace(sample=sample))


def test_latents_to_clip_is_the_expression_it_replaced(monkeypatch):
    monkeypatch.setattr(ops, "clamp01_", lambda x: x.add_(1.0).mul_(0.5).clamp_(0.0, 1.0))     # seer_clamp01 restated for the CPU
    vae = _VAE()
    samples = torch.randn((2, 4, 3, 5, 6), generator=torch.Generator().manual_seed(1)) * 3.0
    n, ch, f, h, w = samples.shape
    z = (samples.permute(0, 2, 1, 3, 4).reshape(n * f, ch, h, w) * (1 / 0.18215)).contiguous()
    x = vae.decode(z).sample
    x = x.reshape(n, f, *x.shape[1:]).permute(0, 2, 1, 3, 4).contiguous()
    want = ops.clamp01_(x.float())
    got = ddim.latents_to_clip(vae, samples)
    assert got.shape == (2, 4, 3, 5, 6) and got.is_contiguous() and torch.equal(got, want)
    assert float(got.min()) == 0.0 and float(got.max()) == 1.0 and 0.0 < float(got.mean()) < 1.0      # both clamps and the middle


def test_frames_to_latents_is_the_expression_it_replaced_and_draws_in_order():
    x0_image = torch.randn((2, 3, 2, 8, 8), generator=torch.Generator().manual_seed(2))
    video = torch.randn((1, 3, 4, 8, 8), generator=torch.Generator().manual_seed(3))
    vae, g = _VAE(), torch.Generator().manual_seed(7)
    want = []
    for clip in (x0_image, video):                        # two consecutive encodes off one generator
        b, f = clip.shape[0], clip.shape[2]
        frames = clip.permute(0, 2, 1, 3, 4).reshape(b * f, *clip.shape[1:2], *clip.shape[3:])    # (b f) c h w
        lat = vae.encode(frames).latent_dist.sample(generator=g) * 0.18215
        want.append(lat.reshape(b, f, *lat.shape[1:]).permute(0, 2, 1, 3, 4).contiguous())       # b c f h w
    ref_draws, vae.draws = vae.draws, []
    g = torch.Generator().manual_seed(7)
    got = [ddim.frames_to_latents(vae, x0_image, g), ddim.frames_to_latents(vae, video, g)]
    for a, b_ in zip(got, want):
        assert a.shape == b_.shape and a.is_contiguous() and torch.equal(a, b_)
    assert len(vae.draws) == 2 and all(torch.equal(a, b_) for a, b_ in zip(vae.draws, ref_draws))
    assert not torch.equal(vae.draws[0].flatten()[:64], vae.draws[1].flatten()[:64])
    # a one-frame image expanded over the conditioning frames (generate_clips): a view goes through like a tensor of its own
    image = x0_image[:, :, :1].expand(-1, -1, 3, -1, -1)
    assert torch.equal(ddim.frames_to_latents(vae, image, torch.Generator().manual_seed(9)),
                       ddim.frames_to_latents(vae, image.contiguous(), torch.Generator().manual_seed(9)))
