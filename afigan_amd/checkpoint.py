"""Weight hand-off between the three training stages (SURVEY.md sections 3.4 and 8(f) row 2).

Host-side restatement of the key remapping of ``AF_DetectionCheckpointer`` (afigan/engine/checkpoint.py:64-125 and the two
``align_and_update_state_dicts_*`` methods, :127-258) as plain functions over state dicts, so stage-1 interpolator weights
(keys ``Generators.0...``) load into an AFI backbone of this package (keys ``backbone.srf_module.Generators.0...``) and a
stage-2 AF-extractor checkpoint hands only its ``srf_module`` tensors to the stage-3 detector.  No GPU work here.
"""
import logging
import pickle
import re
from typing import Dict, List, Tuple

import torch

logger = logging.getLogger(__name__)


def convert_afi_names(weights: Dict[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], Dict[str, str]]:
    """Stage 1 -> stage 2 (checkpoint.py:78-111): every ``Generators`` in a key becomes ``backbone.srf_module.Generators``.
    Returns (renamed weights, renamed key -> original key)."""
    new_weights, new_to_old = {}, {}
    for orig in sorted(weights):
        renamed = orig.replace("Generators", "backbone.srf_module.Generators")
        if renamed in new_weights:
            raise ValueError(f"renaming {orig!r} collides with another key ({renamed!r})")
        new_weights[renamed] = weights[orig]
        new_to_old[renamed] = orig
    return new_weights, new_to_old


def remain_only_afi_names(weights: Dict[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], Dict[str, str]]:
    """Stage 2 -> stage 3 (checkpoint.py:113-125): keep only the tensors whose key mentions ``srf_module``."""
    kept = {k: weights[k] for k in sorted(weights) if "srf_module" in k}
    return kept, {k: k for k in kept}


def align_and_update(model_state_dict: Dict[str, torch.Tensor], ckpt_state_dict: Dict[str, torch.Tensor]) -> Dict[str, str]:
    """The suffix matching shared by both loaders (checkpoint.py:127-197 / :199-258): a model key takes the checkpoint key
    that equals it or is its longest complete ``.``-suffix; a shape mismatch skips the pair with a warning; one checkpoint key
    feeding two model keys is an error.  Updates ``model_state_dict`` in place (clones) and returns {ckpt key: model key}."""
    model_keys, ckpt_keys = sorted(model_state_dict), sorted(ckpt_state_dict)
    matched: Dict[str, str] = {}
    for mk in model_keys:
        best, best_len = None, 0
        for ck in ckpt_keys:
            if (mk == ck or mk.endswith("." + ck)) and len(ck) > best_len:      # first longest match, as torch.max returns
                best, best_len = ck, len(ck)
        if best is None:
            continue
        value = ckpt_state_dict[best]
        if tuple(model_state_dict[mk].shape) != tuple(value.shape):
            logger.warning("Shape of %s in checkpoint is %s, while shape of %s in model is %s; not loaded.", best, tuple(value.shape),
                           mk, tuple(model_state_dict[mk].shape))
            continue
        model_state_dict[mk] = value.clone()
        if best in matched:
            raise ValueError(f"Cannot match one checkpoint key to multiple keys in the model: {best} -> {mk} and {matched[best]}")
        matched[best] = mk
    return matched


def _model_dict(checkpoint):
    return checkpoint["model"] if isinstance(checkpoint, dict) and "model" in checkpoint else checkpoint


def load_af_extractor_weights(model: torch.nn.Module, checkpoint) -> Dict[str, str]:
    """``_load_AFExtractor_weights_file`` (checkpoint.py:64-69) on an already-read checkpoint (``{"model": ...}`` or a bare
    state dict): stage-1 interpolator weights into ``model``'s ``backbone.srf_module``."""
    sd = model.state_dict()
    renamed, _ = convert_afi_names(_model_dict(checkpoint))
    matched = align_and_update(sd, renamed)
    model.load_state_dict(sd, strict=True)
    return matched


def load_target_detector_weights(model: torch.nn.Module, checkpoint) -> Dict[str, str]:
    """``_load_TargetDetector_weights_file`` (checkpoint.py:71-76): only the ``srf_module`` tensors of a stage-2 checkpoint."""
    sd = model.state_dict()
    kept, _ = remain_only_afi_names(_model_dict(checkpoint))
    matched = align_and_update(sd, kept)
    model.load_state_dict(sd, strict=True)
    return matched


# Caffe2 / Detectron1 blob names (ImageNet R-50.pkl, Detectron1 model zoo): detectron2 loads them only through its name-matching heuristics,
# which the reference's guide loader never runs (stage1_trainer.py:62-74 calls _load_model on the raw pickle)
_CAFFE2_NAME = re.compile(r"^(conv1_[wb]|res_conv1_bn_[sb]|res\d+_\d+_branch\w+|fpn_inner_\w+|fpn_res\d+\w*|pred_\w+)$")


def read_guide_checkpoint(path) -> Dict[str, torch.Tensor]:
    """The state dict of a guide checkpoint file: a detectron2 model-zoo ``.pkl`` (``{"model": {name: numpy array}, "__author__": ...}``,
    read with ``pickle.load(..., encoding="latin1")`` as stage1_trainer.py:66-68 does) or a ``.pth`` (``{"model": ...}`` or a bare state
    dict).  Caffe2-named files are refused."""
    if str(path).endswith(".pkl"):
        with open(path, "rb") as f:
            data = pickle.load(f, encoding="latin1")
    else:
        data = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(data, dict) and "blobs" in data:
        data = data["blobs"]
    sd = _model_dict(data)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state dict ({type(sd).__name__})")
    caffe2 = sorted(k for k in sd if _CAFFE2_NAME.match(str(k)))
    if caffe2:
        raise ValueError(f"{path}: Caffe2-named weights ({', '.join(caffe2[:3])}, ...) are not supported; use a detectron2-format checkpoint "
                         "(keys like backbone.bottom_up.res2.0.conv1.weight)")
    out = {}
    for k, v in sd.items():
        if k.startswith("module."):                                      # (DDP prefix, stripped as detectron2's Checkpointer does)
            k = k[len("module."):]
        if isinstance(v, torch.Tensor):
            out[k] = v
        elif hasattr(v, "dtype") and hasattr(v, "shape"):                # numpy arrays of a model-zoo pickle
            out[k] = torch.as_tensor(v)
    return out


def load_guide_weights(model: torch.nn.Module, path) -> Tuple[List[str], List[str]]:
    """``_load_model`` of the guide (stage1_trainer.py:62-74): load a guide checkpoint (a path, see read_guide_checkpoint, or an already
    read state dict) NON-strictly into ``model`` (``RCNN_FPN_only``: keys ``backbone.*``).  Every key present on both sides must have the
    same shape (ValueError otherwise).  Returns (missing keys: in the model, not in the file; unused keys: in the file, not in the model)."""
    sd = model.state_dict()
    ckpt = read_guide_checkpoint(path) if not isinstance(path, dict) else {k: torch.as_tensor(v) for k, v in _model_dict(path).items()}
    bad = [(k, tuple(v.shape), tuple(sd[k].shape)) for k, v in ckpt.items() if k in sd and tuple(v.shape) != tuple(sd[k].shape)]
    if bad:
        raise ValueError("guide checkpoint shapes do not match the model: " + "; ".join(f"{k}: file {a}, model {b}" for k, a, b in bad[:5]))
    matched = {k: v for k, v in ckpt.items() if k in sd}
    model.load_state_dict(matched, strict=False)
    missing = sorted(k for k in sd if k not in ckpt)
    unused = sorted(k for k in ckpt if k not in sd)
    if missing:
        logger.warning("guide checkpoint: %d model keys not in the file (first: %s)", len(missing), missing[0])
    return missing, unused
