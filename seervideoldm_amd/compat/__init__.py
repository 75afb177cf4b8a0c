"""Run the reference's scripts UNCHANGED on the MI355X path.

`inference_img.py`, `eval.py`, `inference.py` and `train.py` import the hot path by three module names
(inference_img.py:29,38-39):

    from seer.models.unet_3d_condition import SeerUNet, FSTextTransformer
    from ldm.models.diffusion.ddim_video import DDIMSampler
    from utils.ddim_sampling_utils import ddim_sample, save_visualization_onegif

`install()` puts a finder in front of `sys.meta_path` that answers exactly those three names with modules that re-export
the product classes (same names, arguments and return values: SURVEY 8(b)).  Every other module of the reference checkout
(`utils.fvd`, `ldm.util`, datasets ...) still resolves to the reference's own file, because the parent packages are
presented as namespace packages over the directories found on `sys.path`.

    python -m seervideoldm_amd.compat inference_img.py --config configs/inference_base.yaml ...

runs the script with the aliases installed (`sys.argv`, `sys.path[0]` and `__main__` as `python script.py` sets them).
`install(vae=True)` (or `SEER_COMPAT_VAE=1` with the runner) also replaces `diffusers.AutoencoderKL` by the product's VAE
when `diffusers` is importable; without it the reference keeps its fp32 torch VAE for `vae.decode` / `vae.encode`.
`SEER_COMPAT_SAMPLER=plms` (read by `install()`) makes the scripts sample with `PLMSSampler` under the name `DDIMSampler`: the
yaml's `ddim_steps` is then the PLMS step count (S steps cost S + 1 UNet evaluations).  `SEER_COMPAT_SAMPLER=dpmpp` makes it
`DPMSolverSampler` (DPM-Solver++ 2M with its defaults, one evaluation per step; INTEGRATION.md says which `ddim_steps` to pick).
`SEER_COMPAT_PREDICTION=v_prediction` (read by `install()`, or `install(prediction="v_prediction")`) makes that sampler, whichever it
is, treat the UNet's output as the velocity v (a model fine-tuned with `prediction_type: v_prediction`, train.py:373-374); unset or
`epsilon`, it is eps as before.
`SEER_COMPAT_GUIDANCE_RESCALE=0.7` (read by `install()`, or `install(guidance_rescale=0.7)`) makes that sampler rescale its guided
output to the conditional branch's std, blended by that factor (Lin et al. 2023; a number in [0, 1], how v-models are sampled);
unset or 0, nothing is rescaled.
`SEER_COMPAT_FREEU="0.9,0.2,1.2,1.4"` (read by `install()`, or `install(freeu=(0.9, 0.2, 1.2, 1.4))`: s1, s2, b1, b2 in diffusers'
order) makes the aliased `SeerUNet` one that comes with FreeU enabled at those values (`SeerUNet.enable_freeu`; Si et al. 2024);
unset or empty, the class is the product's own.  Inference scripts only: `SeerTrainer` refuses such a model.
`SEER_COMPAT_STEP_CACHE="3,1,1"` (read by `install()`, or `install(step_cache=(3, 1, 1))`: interval, branch, order) makes the aliased
`SeerUNet` one that comes with step caching enabled (`SeerUNet.enable_step_cache`; DeepCache, Ma et al. 2024): the scripts' sampler
then runs every interval-th model evaluation in full and the others from the cached feature.  Unset or empty, nothing is cached.
`SEER_COMPAT_CLIP=native` (read by `install()`, or `install(clip="native")`) makes `transformers.CLIPTextModel` the product's
`CLIPTextEncoder` (train.py:21,199; inference_img.py:85): `CLIPTextModel.from_pretrained(<local directory>, subfolder="text_encoder")`
then loads the text tower onto the HIP kernels.  Unset, the scripts keep transformers' module.
"""
from __future__ import annotations

import importlib.abc
import importlib.machinery
import os
import sys
import types
from typing import Optional

ALIASES = {
    "seer.models.unet_3d_condition": "seervideoldm_amd.compat._unet_3d_condition",
    "ldm.models.diffusion.ddim_video": "seervideoldm_amd.compat._ddim_video",
    "utils.ddim_sampling_utils": "seervideoldm_amd.compat._ddim_sampling_utils",
}
_PARENTS = sorted({".".join(n.split(".")[:i]) for n in ALIASES for i in range(1, n.count(".") + 1)})


class _AliasFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path=None, target=None):
        if fullname in ALIASES:
            return importlib.machinery.ModuleSpec(fullname, self)
        if fullname in _PARENTS:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        if spec.name in ALIASES:
            src = importlib.import_module(ALIASES[spec.name])
            mod = types.ModuleType(spec.name, src.__doc__)
            mod.__dict__.update({k: v for k, v in src.__dict__.items() if not k.startswith("__")})
            mod.__all__ = list(getattr(src, "__all__", []))
            if spec.name == "ldm.models.diffusion.ddim_video" and _sampler == "plms":
                from seervideoldm_amd.plms import PLMSSampler
                mod.DDIMSampler = PLMSSampler
            if spec.name == "ldm.models.diffusion.ddim_video" and _sampler == "dpmpp":
                from seervideoldm_amd.dpm import DPMSolverSampler
                mod.DDIMSampler = DPMSolverSampler
            if spec.name == "ldm.models.diffusion.ddim_video" and _prediction == "v_prediction":
                mod.DDIMSampler = _v_sampler(mod.DDIMSampler)
            if spec.name == "ldm.models.diffusion.ddim_video" and _rescale:
                mod.DDIMSampler = _rescale_sampler(mod.DDIMSampler, _rescale)
            if spec.name == "seer.models.unet_3d_condition" and _freeu is not None:
                mod.SeerUNet = _freeu_unet(mod.SeerUNet, _freeu)
            if spec.name == "seer.models.unet_3d_condition" and _step_cache is not None:
                mod.SeerUNet = _step_cache_unet(mod.SeerUNet, _step_cache)
            return mod
        # a parent package: a namespace over every directory of that name on sys.path (the reference checkout's own
        # `utils/`, `ldm/`, `seer/` when the script runs from there), so the reference's other modules keep resolving
        mod = types.ModuleType(spec.name)
        rel = spec.name.replace(".", os.sep)
        mod.__path__ = [os.path.join(p or os.getcwd(), rel) for p in sys.path if os.path.isdir(os.path.join(p or os.getcwd(), rel))]
        # submodules that were imported before install() stay importable as attributes of the new package object
        for name, sub in list(sys.modules.items()):
            if name.startswith(spec.name + ".") and "." not in name[len(spec.name) + 1:] and name not in ALIASES and name not in _PARENTS:
                setattr(mod, name.rsplit(".", 1)[1], sub)
        return mod

    def exec_module(self, module):
        pass


_finder = _AliasFinder()
_sampler = None
_prediction = None
_v_samplers = {}            # sampler class -> its subclass whose prediction_type defaults to "v_prediction": one per class


def _v_sampler(cls):
    """`cls` with prediction_type="v_prediction" as its constructor's default: the scripts build their sampler without the keyword"""
    if cls not in _v_samplers:
        def __init__(self, *args, **kwargs):
            kwargs.setdefault("prediction_type", "v_prediction")
            cls.__init__(self, *args, **kwargs)
        _v_samplers[cls] = type(cls.__name__, (cls,), {"__init__": __init__, "__doc__": cls.__doc__, "__module__": cls.__module__})
    return _v_samplers[cls]


_rescale = 0.
_rescale_samplers = {}      # (sampler class, phi) -> its subclass whose guidance_rescale defaults to phi


def _rescale_sampler(cls, phi: float):
    """`cls` with guidance_rescale=phi as its constructor's default, as _v_sampler does for the prediction type"""
    if (cls, phi) not in _rescale_samplers:
        def __init__(self, *args, **kwargs):
            kwargs.setdefault("guidance_rescale", phi)
            cls.__init__(self, *args, **kwargs)
        _rescale_samplers[cls, phi] = type(cls.__name__, (cls,), {"__init__": __init__, "__doc__": cls.__doc__,
                                                                  "__module__": cls.__module__})
    return _rescale_samplers[cls, phi]


_freeu = None               # (s1, s2, b1, b2) while the aliased SeerUNet comes with FreeU enabled
_freeu_unets = {}           # (SeerUNet class, values) -> its subclass whose instances have FreeU enabled at those values


def _parse_freeu(text):
    """"s1,s2,b1,b2" -> four finite floats; a ValueError that names the variable otherwise"""
    try:
        vals = tuple(float(v) for v in text.split(","))
    except ValueError:
        vals = ()
    if len(vals) != 4 or any(v != v or v in (float("inf"), float("-inf")) for v in vals):
        raise ValueError(f"SEER_COMPAT_FREEU={text!r}: four finite numbers s1,s2,b1,b2, such as 0.9,0.2,1.2,1.4")
    return vals


def _freeu_unet(cls, vals):
    """`cls` whose constructor ends with enable_freeu(*vals), as _v_sampler does for the prediction type"""
    if (cls, vals) not in _freeu_unets:
        def __init__(self, *args, **kwargs):
            cls.__init__(self, *args, **kwargs)
            self.enable_freeu(*vals)
        _freeu_unets[cls, vals] = type(cls.__name__, (cls,), {"__init__": __init__, "__doc__": cls.__doc__, "__module__": cls.__module__})
    return _freeu_unets[cls, vals]


_step_cache = None          # (interval, branch, order) while the aliased SeerUNet comes with step caching enabled
_step_cache_unets = {}      # (SeerUNet class, values) -> its subclass whose instances have step caching enabled at those values


def _parse_step_cache(text):
    """"interval,branch,order" -> three integers; a ValueError that names the variable otherwise (the ranges are enable_step_cache's)"""
    try:
        vals = tuple(int(v) for v in text.split(","))
    except ValueError:
        vals = ()
    if len(vals) != 3 or vals[0] < 2 or vals[1] < 0 or vals[2] not in (0, 1, 2):
        raise ValueError(f"SEER_COMPAT_STEP_CACHE={text!r}: three integers interval,branch,order with interval >= 2, branch >= 0 and "
                         "order 0, 1 or 2, such as 3,1,1")
    return vals


def _step_cache_unet(cls, vals):
    """`cls` whose constructor ends with enable_step_cache(*vals), as _freeu_unet does for FreeU"""
    if (cls, vals) not in _step_cache_unets:
        def __init__(self, *args, **kwargs):
            cls.__init__(self, *args, **kwargs)
            self.enable_step_cache(*vals)
        _step_cache_unets[cls, vals] = type(cls.__name__, (cls,), {"__init__": __init__, "__doc__": cls.__doc__,
                                                                   "__module__": cls.__module__})
    return _step_cache_unets[cls, vals]


_clip_saved = None          # (transformers module, its own CLIPTextModel) while the native text encoder stands in


def install(vae: bool = False, sampler: Optional[str] = None, clip: Optional[str] = None,
            prediction: Optional[str] = None, guidance_rescale: Optional[float] = None, freeu=None, step_cache=None) -> None:
    """`sampler` (default: the environment's SEER_COMPAT_SAMPLER) = "plms" makes the aliased
    `ldm.models.diffusion.ddim_video.DDIMSampler` the product's PLMSSampler, "dpmpp" its DPMSolverSampler; anything else keeps
    DDIMSampler.
    `prediction` (default: the environment's SEER_COMPAT_PREDICTION) = "v_prediction" makes that class one whose constructor defaults
    to prediction_type="v_prediction"; "epsilon" or nothing keeps it as it is; anything else is train.py:376's ValueError.
    `guidance_rescale` (default: the environment's SEER_COMPAT_GUIDANCE_RESCALE, 0 when unset) in (0, 1] makes that class one whose
    constructor defaults to guidance_rescale of that value; 0 keeps it as it is; anything outside [0, 1] is a ValueError.
    `freeu` (default: the environment's SEER_COMPAT_FREEU, "s1,s2,b1,b2") = four finite numbers makes the aliased SeerUNet a class whose
    instances have FreeU enabled at those values; nothing keeps the class as it is; malformed text is a ValueError naming the variable.
    `step_cache` (default: the environment's SEER_COMPAT_STEP_CACHE, "interval,branch,order") = three integers makes the aliased SeerUNet
    a class whose instances have step caching enabled at those values; nothing keeps the class as it is; malformed text is a ValueError
    naming the variable.
    `clip` (default: the environment's SEER_COMPAT_CLIP) = "native" makes `transformers.CLIPTextModel` the product's
    CLIPTextEncoder until uninstall(); anything else leaves transformers alone"""
    global _sampler, _prediction, _rescale, _clip_saved, _freeu, _step_cache
    _sampler = (os.environ.get("SEER_COMPAT_SAMPLER", "") if sampler is None else sampler).strip().lower()
    _prediction = (os.environ.get("SEER_COMPAT_PREDICTION", "") if prediction is None else prediction).strip().lower()
    if _prediction not in ("", "epsilon", "v_prediction"):
        raise ValueError(f"Unknown prediction type {_prediction}")
    from seervideoldm_amd.ops import check_guidance_rescale
    _rescale = check_guidance_rescale((os.environ.get("SEER_COMPAT_GUIDANCE_RESCALE", "").strip() or 0.)
                                      if guidance_rescale is None else guidance_rescale)
    if freeu is None:
        text = os.environ.get("SEER_COMPAT_FREEU", "").strip()
        _freeu = _parse_freeu(text) if text else None
    else:
        _freeu = _parse_freeu(",".join(repr(float(v)) for v in freeu))
    if step_cache is None:
        text = os.environ.get("SEER_COMPAT_STEP_CACHE", "").strip()
        _step_cache = _parse_step_cache(text) if text else None
    else:
        _step_cache = _parse_step_cache(",".join(str(v) for v in step_cache))
    if (os.environ.get("SEER_COMPAT_CLIP", "") if clip is None else clip).strip().lower() == "native" and _clip_saved is None:
        import transformers
        from seervideoldm_amd import CLIPTextEncoder
        _clip_saved = (transformers, transformers.CLIPTextModel)
        transformers.CLIPTextModel = CLIPTextEncoder
    if _finder not in sys.meta_path:
        sys.meta_path.insert(0, _finder)
    for name in list(ALIASES) + _PARENTS:      # modules imported before install() (the reference's own) give way
        sys.modules.pop(name, None)
    if vae:
        try:
            import diffusers
        except ImportError:
            return
        from seervideoldm_amd import AutoencoderKL
        diffusers.AutoencoderKL = AutoencoderKL


def uninstall() -> None:
    global _clip_saved
    if _clip_saved is not None:
        _clip_saved[0].CLIPTextModel = _clip_saved[1]
        _clip_saved = None
    if _finder in sys.meta_path:
        sys.meta_path.remove(_finder)
    for name in list(ALIASES) + _PARENTS:
        sys.modules.pop(name, None)
