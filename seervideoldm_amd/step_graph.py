"""What the captured steps of DDIMSampler / PLMSSampler (ddim.py, plms.py) and SlotSampler (slots.py) share on the host: whether a
model's steps may be captured at all (capture_engine), whether a caller has brought new tensors for static buffers (changed /
refresh), and the capture itself (capture_step).  A step's kind, key, buffers and launches stay with the sampler that steps."""
import torch

from . import ops


def engine_on(unet, device):
    """the SeerUNet's engine on `device`, built when it is missing or lives on another device"""
    if unet._engine is None or unet._engine.device != device:
        unet.prepare()
    return unet._engine


def capture_engine(unet, backend, device):
    """The engine to capture a sampler step on, or None when no step of this model may be captured: it takes an unsharded SeerUNet
    without center_input_sample that replays graphs (unet.use_graph), the HIP backend on the model's side and the sampler's
    (`backend`), a GPU, and an engine no capture has failed on.  A sampler adds its own refusal flag and what depends on the step."""
    from .unet import SeerUNet
    if not isinstance(unet, SeerUNet) or unet._shard is not None or unet.config.center_input_sample or not unet.use_graph \
            or backend is not ops or unet._ops_backend is not ops or device.type != "cuda":
        return None
    eng = engine_on(unet, device)
    return None if getattr(eng, "_graph_broken", False) else eng


def changed(kept: dict, name: str, sources) -> bool:
    """Are `sources` other tensors than at the last call under `name`, or written since?  A tensor is recognised by its identity and
    its (data_ptr, _version).  `kept` holds the tensors beside that key and so keeps them alive: the address of a freed tensor handed
    to the next sample's tensor must not look like "unchanged"."""
    key = tuple((s.data_ptr(), s._version) for s in sources)
    last = kept.get(name)
    if last is not None and last[0] == key and all(a is b for a, b in zip(last[1], sources)):
        return False
    kept[name] = (key, tuple(sources))
    return True


def refresh(kept: dict, name: str, sources, dests) -> bool:
    """static buffers that a captured step reads by address: when any of `sources` changed since the last call under `name`, copy
    them all into `dests` (they belong together).  Returns whether it copied."""
    if not changed(kept, name, sources):
        return False
    for s, d in zip(sources, dests):
        d.copy_(s)
    return True


def capture_step(eng, key, G, body, cached_body=None):
    """`body` (the launches of one sampler step over the static buffers in G) as ONE hipGraph: a warm-up run, the capture, and the
    entry G -- with the graph under "graph" -- in the engine's graph cache under `key`.  Returns G, or None with a warning when the
    capture is refused: the caller keeps the launch-by-launch path.  `cached_body` (step caching): the same step around a cached
    model evaluation, over the SAME static buffers, as a second graph under "graph_cached" in the same entry and the first one's
    memory pool (the two never run at once and hand nothing to each other but G); both are captured or neither is."""
    try:
        graphs = []
        for b in (body,) if cached_body is None else (body, cached_body):
            b()                                      # warm-up: K|V / rotary caches, allocations
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local", **({"pool": graphs[0].pool()} if graphs else {})):
                b()
            graphs.append(g)
    except Exception as e:      # noqa: BLE001  capture refused: keep the launch-by-launch path
        import warnings
        warnings.warn(f"hipGraph capture of the sampler step failed ({type(e).__name__}: {e}); stepping launch by launch")
        return None
    G["graph"] = graphs[0]
    if cached_body is not None:
        G["graph_cached"] = graphs[1]
    eng.graph_put(key, G)
    return G
