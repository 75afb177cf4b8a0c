"""TEST INFRASTRUCTURE ONLY -- step caching (SeerUNet.enable_step_cache; seer_cache_push / seer_cache_forecast) restated from its
definition for tests/test_step_cache_host.py and tests/test_gpu_step_cache.py.

    push_ref(ring, x)                         the ring [3, stride] after one push of x, on the bits
    forecast64(slots, w)                      w0 f0 + w1 f1 + w2 f2 in float64 (the exact constructions)
    forecast_ref(slots, w, dtype)             the kernel's fixed fp32 order -- w0 * f0, then two fmaf -- emulated in float64 (exact
                                              where each product and sum fits 53 bits), one rounding to the storage type; a slot
                                              whose weight is 0 is not read
    weights(d, interval, order, valid)        the table of the issue, float64 -> fp32
    full_walk(sd, cfg, ..., branch)           the oracle's forward built from its blocks, recording the cut feature
    cached_walk(sd, cfg, ..., branch, feat)   the cached evaluation: conv_in, `branch` layers of down_blocks.0, the layers
                                              L - branch .. L of the last up block from `feat`, conv_norm_out, conv_out
    TorchOpsWithStepCache / Recording         tests/torch_ops_backend.py plus cache_push / cache_forecast (that file is not edited)
    RecordingWeights                          a mapping over the engine's packed weights that writes down every key it is asked for
"""
import torch
import torch.nn.functional as F

from oracle import seer_oracle as O
from tests import torch_ops_backend as tob


# ---- the two kernels ------------------------------------------------------------------------------------------------------------------
def push_ref(ring, x):
    """ring [3, stride] and x [n] of one 16-bit type -> the ring after slot2 <- slot1 <- slot0 <- x over the first n elements"""
    n = x.numel()
    out = ring.clone()
    bits, xb = out.view(torch.int16), x.reshape(-1).view(torch.int16)
    old = ring.view(torch.int16)
    bits[2, :n], bits[1, :n], bits[0, :n] = old[1, :n], old[0, :n], xb
    return out


def forecast64(slots, w):
    return sum(float(wk) * f.double() for wk, f in zip(w, slots))


def _f32(x64):
    return x64.to(torch.float32).double()


def forecast_ref(slots, w, dtype):
    """slots: three tensors of the storage type; w: three fp32 values.  acc = w0 * f0, acc = fmaf(w1, f1, acc), acc = fmaf(w2, f2,
    acc), each one float64 operation rounded once to fp32; then one rounding to `dtype`.  Zero weights skip their slot."""
    w = [float(torch.tensor(v, dtype=torch.float32)) for v in w]
    acc = torch.zeros(slots[0].shape, dtype=torch.float64)
    for k, (wk, f) in enumerate(zip(w, slots)):
        if wk == 0.0:
            continue
        acc = _f32(wk * f.double() + (acc if k else 0.0))
    return acc.to(torch.float32).to(dtype)


def weights(d, interval, order, valid):
    u = d / interval
    o = min(order, valid - 1)
    q = u * (u + 1.0)
    w = [(1.0, 0.0, 0.0), (1.0 + u, -u, 0.0), (1.0 + u + q / 2.0, -u - q, q / 2.0)][o]
    return tuple(float(torch.tensor(v, dtype=torch.float64).to(torch.float32)) for v in w)


# ---- the two walks, from the oracle's blocks -----------------------------------------------------------------------------------------
def _setup(sd, cfg, sample, timestep, context, cond_frame):
    c = dict(O.DEFAULT_CFG)
    c.update(cfg)
    boc, L, heads = tuple(c["block_out_channels"]), c["layers_per_block"], c["attention_head_dim"]
    G, eps = c["norm_num_groups"], c["norm_eps"]
    t = timestep.broadcast_to(sample.shape[0])
    emb = O.timestep_embedding(t, boc[0], c["flip_sin_to_cos"], c["freq_shift"])
    emb = O._lin(sd, "time_embedding.linear_2", F.silu(O._lin(sd, "time_embedding.linear_1", emb)))

    def layer(p, j, x, attn=True):
        x = O.resnet_block(sd, f"{p}.resnets.{j}", x, emb, G, eps)
        if attn:
            x = O.spatial_transformer(sd, f"{p}.attentions.{j}", x, context, heads, False, cond_frame, G)
            x = O.spatial_transformer(sd, f"{p}.temporal_attentions.{j}", x, None, heads, True, cond_frame, G)
        return x

    def head(x):
        return O.conv_frames(sd, "conv_out", F.silu(O.group_norm5d(sd, "conv_norm_out", x, G, eps)))
    return len(boc), L, layer, head, emb, G, eps, heads


def full_walk(sd, cfg, sample, timestep, context, cond_frame, branch):
    """-> (output, cut feature [B, boc[0], F, H, W]): unet_forward written out, the backbone input of up_blocks.{n-1}.resnets.{L -
    branch} kept on the way"""
    n, L, layer, head, emb, G, eps, heads = _setup(sd, cfg, sample, timestep, context, cond_frame)
    x = O.conv_frames(sd, "conv_in", sample)
    skips = [x]
    for i in range(n):
        for j in range(L):
            x = layer(f"down_blocks.{i}", j, x, attn=i < n - 1)
            skips.append(x)
        if i < n - 1:
            x = O.conv_frames(sd, f"down_blocks.{i}.downsamplers.0.conv", x, stride=2, padding=1)
            skips.append(x)
    x = O.resnet_block(sd, "mid_block.resnets.0", x, emb, G, eps)
    x = O.spatial_transformer(sd, "mid_block.attentions.0", x, context, heads, False, cond_frame, G)
    x = O.spatial_transformer(sd, "mid_block.temporal_attentions.0", x, None, heads, True, cond_frame, G)
    x = O.resnet_block(sd, "mid_block.resnets.1", x, emb, G, eps)
    feat = None
    for i in range(n):
        for j in range(L + 1):
            if i == n - 1 and j == L - branch:
                feat = x.clone()
            x = layer(f"up_blocks.{i}", j, torch.cat([x, skips.pop()], dim=1), attn=i > 0)
        if i < n - 1:
            x = O.upsample(sd, f"up_blocks.{i}.upsamplers.0", x)
    return head(x), feat


def cached_walk(sd, cfg, sample, timestep, context, cond_frame, branch, feat):
    n, L, layer, head, *_ = _setup(sd, cfg, sample, timestep, context, cond_frame)
    x = O.conv_frames(sd, "conv_in", sample)
    skips = [x]
    for j in range(branch):
        x = layer("down_blocks.0", j, x)
        skips.append(x)
    x = feat
    for j in range(L - branch, L + 1):
        x = layer(f"up_blocks.{n - 1}", j, torch.cat([x, skips.pop()], dim=1))
    return head(x)


def skipped_prefixes(n, L, branch):
    """the module paths a cached evaluation with `branch` must not touch"""
    skipped = ["down_blocks.0.downsamplers.", "mid_block."]
    skipped += [f"down_blocks.{i}." for i in range(1, n)] + [f"up_blocks.{i}." for i in range(n - 1)]
    for kind in ("resnets", "attentions", "temporal_attentions"):
        skipped += [f"down_blocks.0.{kind}.{j}." for j in range(branch, L)]
        skipped += [f"up_blocks.{n - 1}.{kind}.{j}." for j in range(L - branch)]
    return tuple(skipped)


# ---- the stand-in backend ------------------------------------------------------------------------------------------------------------
class TorchOpsWithStepCache:
    """tests/torch_ops_backend.py with `cache_push` and `cache_forecast` added -- and the two things a layout-invariant engine asks
    of its backend that the stand-in lacks: the row count from which the 320-channel row-owner launches pay (the product's value; the
    stand-in has neither launch, so it only has to be a number) and conv_out's tile request, which a torch conv has no use for"""
    FF_FUSED_MIN_ROWS = 18432

    def __getattr__(self, name):
        return getattr(tob, name)

    def conv_out(self, *a, tile=0, **k):
        return tob.conv_out(*a, **k)

    def cache_push(self, x, ring):
        ring.copy_(push_ref(ring, x))

    def cache_forecast(self, ring, w, out):
        n = out.numel()
        out.copy_(forecast_ref([ring[k, :n] for k in range(3)], w.tolist(), out.dtype).reshape(out.shape))
        return out


class RecordingStepCache(TorchOpsWithStepCache):
    """... and every call written down: ("push", n) / ("forecast", n, weights)"""

    def __init__(self):
        self.calls = []

    def cache_push(self, x, ring):
        self.calls.append(("push", x.numel()))
        super().cache_push(x, ring)

    def cache_forecast(self, ring, w, out):
        self.calls.append(("forecast", out.numel(), tuple(w.tolist())))
        return super().cache_forecast(ring, w, out)


class RecordingWeights(dict):
    """the engine's `w` with every key it is asked for -- by [], .get or `in` -- written down"""

    def __init__(self, w):
        super().__init__(w)
        self.touched = []

    def __getitem__(self, k):
        self.touched.append(k)
        return super().__getitem__(k)

    def get(self, k, default=None):
        self.touched.append(k)
        return super().get(k, default)

    def __contains__(self, k):
        self.touched.append(k)
        return super().__contains__(k)
