"""Writes tests/golden/clip_text_tiny.npz from the INSTALLED transformers.CLIPTextModel (no download: the model is built from a
CLIPTextConfig):  python -m tests.make_clip_golden

hidden 128 (2 heads of 64), intermediate 128, 2 layers, vocab 64, 77 positions; transformers' own initialisation plus N(0, 0.1) on
every 1-D parameter, so that biases and LayerNorm gains are not trivial.  Every parameter is then rounded to the fp16 grid BEFORE
the model runs: the fixture stores them as fp16 without loss, which halves the file (0.47 MB instead of 0.95 MB of weights; the
outputs stay fp32).  Five samples of 77 tokens: prefix masks of lengths 1, 2, 20 and 77 and one mask with holes (keys 5..8 off);
key 0 is visible in all of them.  Keys carry the checkpoint's `text_model.` prefix whatever the installed version calls them."""
from pathlib import Path

import numpy as np
import torch

CFG = dict(vocab_size=64, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
           max_position_embeddings=77, layer_norm_eps=1e-5, hidden_act="quick_gelu")
OUT = Path(__file__).parent / "golden" / "clip_text_tiny.npz"


def inputs():
    g = torch.Generator().manual_seed(1234)
    ids = torch.randint(0, CFG["vocab_size"], (5, 77), generator=g)
    mask = torch.zeros((5, 77), dtype=torch.int64)
    for i, n in enumerate((1, 2, 20, 77)):
        mask[i, :n] = 1
    mask[4] = 1
    mask[4, 5:9] = 0
    return ids, mask


def main():
    from transformers import CLIPTextConfig, CLIPTextModel
    torch.manual_seed(0)
    model = CLIPTextModel(CLIPTextConfig(**CFG)).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            p.copy_(p.to(torch.float16).float())
    ids, mask = inputs()
    with torch.no_grad():
        out = model(ids, attention_mask=mask)[0]
    arrays = {"ids": ids.numpy(), "mask": mask.numpy(), "out": out.float().numpy()}
    for k, v in model.state_dict().items():
        if v.is_floating_point():
            arrays[k if k.startswith("text_model.") else "text_model." + k] = v.to(torch.float16).numpy()
    np.savez_compressed(OUT, **arrays)
    print(OUT, OUT.stat().st_size, "bytes", len(arrays), "arrays")


if __name__ == "__main__":
    main()
