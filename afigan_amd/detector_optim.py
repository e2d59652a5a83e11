"""The detector's optimiser step on HIP: detectron2 v0.1.1's ``build_optimizer`` groups and ``WarmupMultiStepLR`` over one
afi_detector_sgd_step launch, the trainer loop around it, and the step-3 meta-architecture.

  * ``DetectorOptim`` -- torch.optim.SGD as ``build_optimizer`` configures it (solver/build.py: per-parameter groups by key: ``norm.weight`` /
    ``norm.bias`` take WEIGHT_DECAY_NORM, other ``.bias`` keys BASE_LR * BIAS_LR_FACTOR and WEIGHT_DECAY_BIAS, the rest BASE_LR and
    WEIGHT_DECAY; the parameters of ``nn.LayerNorm`` modules take WEIGHT_DECAY_NORM by module type, whatever their key: a Swin's norm1 /
    norm2 / norm{i}), every group's rate under one warm-up / multi-step factor.  ``zero_grad()`` / ``step()``: it drops into
    ``Stage2Step(optimizer=...)``.  One kernel updates every parameter that has a gradient and, for the trainable bias-free convs of a
    ``resnet_guide.ResNet`` or a ``resnest_backbone.ResNeSt``, writes the FrozenBN-folded weight beside the new one, so the next forward
    finds its prepared weights current instead of refolding all convs in torch fp64 (a ResNeSt's tiny fc1 / fc2, whose fold depends on a
    trainable bias, sit in a prepared slot of their own that the module refolds itself).
  * ``DetectorStep`` -- detectron2's ``SimpleTrainer.run_step`` (the reference's ``Target_Detector_Trainer``, step 3).
  * ``GeneralizedRCNN`` -- the step-3 detector: ``GeneralizedRCNN_AFExtractor`` on ``image`` / ``instances``, returning the loss dict alone.

Out of scope (AfiError by key): SOLVER.NESTEROV, SOLVER.CLIP_GRADIENTS.  Gradient exchange between ranks is the caller's (as in Stage2Step)."""
from typing import Dict, Sequence

import numpy as np
import torch

from . import ops
from ._lib import AfiError, DetSgdDesc
from .frozen import cfg_get
from .rcnn_extractor import META_ARCH_REGISTRY, GeneralizedRCNN_AFExtractor, _Images
from .rcnn_only import pad_to_batch
from .stage1 import warmup_multistep_lr


def param_group(name, base_lr=0.001, weight_decay=1e-4, weight_decay_norm=0.0, bias_lr_factor=1.0, weight_decay_bias=1e-4):
    """(lr, weight_decay) of the parameter called `name`: detectron2 v0.1.1 solver/build.py:build_optimizer."""
    if name.endswith("norm.weight") or name.endswith("norm.bias"):
        return base_lr, weight_decay_norm
    if name.endswith(".bias"):
        return base_lr * bias_lr_factor, weight_decay_bias
    return base_lr, weight_decay


def norm_module_params(model):
    """The parameters build_optimizer gives WEIGHT_DECAY_NORM by MODULE TYPE, which `param_group`'s key suffix misses: those of every
    ``nn.LayerNorm`` (detectron2 v0.1.1's list names it beside the BatchNorm family; here only LayerNorm has keys -- norm1, norm2, norm0 ..
    -- that do not end in ``norm.weight`` / ``norm.bias``)."""
    return [p for m in model.modules() if isinstance(m, torch.nn.LayerNorm) for p in m.parameters(recurse=False)]


def param_groups(named_params, norm_params=(), base_lr=0.001, weight_decay=1e-4, weight_decay_norm=0.0, bias_lr_factor=1.0, weight_decay_bias=1e-4):
    """[(lr, weight_decay)] per (name, parameter): `param_group` by key, except that a parameter among `norm_params` (``norm_module_params``)
    takes the norm group whatever its key."""
    norm_ids = {id(p) for p in norm_params}
    return [(base_lr, weight_decay_norm) if id(p) in norm_ids else
            param_group(n, base_lr, weight_decay, weight_decay_norm, bias_lr_factor, weight_decay_bias) for n, p in named_params]


def _same_layout(a, b):
    return a.shape == b.shape and all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n != 1)


class DetectorOptim:
    """torch.optim.SGD over detectron2's parameter groups and schedule, one launch per step (module docstring).

    `modules`: the modules of the model (``model.modules()``; ``build_detector_optimizer`` passes them).  The trainable
    ``resnet_guide.ResNet`` / ``resnest_backbone.ResNeSt`` bottom-ups among them get their folded weights written by the step.  One that is left out -- the default ``()``
    names none -- is still updated correctly, as plain tensors, but its next forward then refolds every conv: right, and slow."""
    FLAT_GRID = False                    # the (<= 512, ntensors) grid: the flat grid over work units measured the same and needs a prefix table

    def __init__(self, named_params, base_lr: float = 0.001, momentum: float = 0.9, weight_decay: float = 1e-4, weight_decay_norm: float = 0.0,
                 bias_lr_factor: float = 1.0, weight_decay_bias: float = 1e-4, lr_steps: Sequence[int] = (30000,), lr_gamma: float = 0.1,
                 warmup_factor: float = 1e-3, warmup_iters: int = 1000, modules=(), norm_params=()):
        from .resnet_guide import ResNetBase
        named = [(n, p) for n, p in named_params if p.requires_grad]
        if not named:
            raise AfiError("DetectorOptim: no parameter requires grad")
        self.names, self.params = [n for n, _ in named], [p for _, p in named]
        dev = self.params[0].device
        for n, p in named:
            if not p.is_cuda or p.device != dev or p.dtype != torch.float32:
                raise AfiError(f"DetectorOptim: {n} is {p.dtype} on {p.device}; fp32 parameters on one GPU only, there is no CPU fallback")
            if not ops._dense(p):
                raise AfiError(f"DetectorOptim: {n} (shape {tuple(p.shape)}, strides {p.stride()}) is not dense in memory")
        self.base_lr, self.momentum = float(base_lr), float(momentum)
        self.sched = (tuple(lr_steps), lr_gamma, warmup_factor, warmup_iters)
        self.groups = param_groups(named, norm_params, self.base_lr, weight_decay, weight_decay_norm, bias_lr_factor, weight_decay_bias)
        sizes = [p.numel() for p in self.params]
        offs = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 for n in sizes])])             # every segment starts 16-byte aligned
        self._offs = [int(o) for o in offs[:-1]]
        self.flat_mom = torch.zeros(int(offs[-1]), device=dev, dtype=torch.float32)            # one buffer, each segment in its parameter's memory order
        self.modules = [m for m in modules if isinstance(m, ResNetBase) and m._train_stages]      # a trainable ResNet or ResNeSt
        self.iter = 0
        self.relayouts = 0                                                                     # gradients that arrived in other strides than their parameter's
        self.device = dev
        self._units = {}

    # ---- the torch.optim.Optimizer surface Stage2Step / DetectorStep use
    def zero_grad(self, set_to_none: bool = True):
        """torch's default: grads become None, so autograd hands its own tensors over instead of accumulating into zeros."""
        for p in self.params:
            if set_to_none or p.grad is None:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.zero_()

    def lr_factor(self, it=None):
        """The schedule's factor at iteration `it` (default: the next step's): every group's rate is its own base rate times this."""
        return warmup_multistep_lr(1.0, self.iter if it is None else it, *self.sched)

    def group_lrs(self, it=None):
        it = self.iter if it is None else it
        return [warmup_multistep_lr(lr, it, *self.sched) for lr, _ in self.groups]                 # in double; rounded once into the table

    def _unit_count(self, i, n, O, I, k, fold):
        key = (i, fold)
        if key not in self._units:
            self._units[key] = ops.detector_sgd_units(n, O, I, k, fold)
        return self._units[key]

    def step(self, gscale: float = 1.0):
        folds = {}
        for net in self.modules:                                   # _prepare(): a cache hit in the steady state, a full rebuild if a buffer changed
            for w, s64, fw in net.fold_slots():
                folds[id(w)] = (s64, fw)
        lrs = self.group_lrs()
        live = [i for i, p in enumerate(self.params) if p.grad is not None]    # torch skips a parameter without a gradient
        if live:
            table = (DetSgdDesc * len(live))()
            units, keep, written = [], [], []
            mom0 = self.flat_mom.data_ptr()
            for d, i in zip(table, live):
                p, g = self.params[i], self.params[i].grad
                if g.dtype != torch.float32 or g.device != p.device or g.is_sparse:
                    raise AfiError(f"DetectorOptim: the gradient of {self.names[i]} is {g.dtype} on {g.device}; dense fp32 on the parameter's GPU only")
                if not _same_layout(g, p):
                    g2 = torch.empty_strided(p.size(), p.stride(), device=p.device, dtype=torch.float32)
                    g2.copy_(g)
                    keep.append(g2)
                    g = g2
                    self.relayouts += 1
                n = p.numel()
                d.p, d.g, d.m, d.n = p.data_ptr(), g.data_ptr(), mom0 + 4 * self._offs[i], n
                d.lr, d.wd = lrs[i], self.groups[i][1]
                slot = folds.get(id(p))
                if slot is not None:
                    s64, fw = slot
                    O, I, k = (p.shape[0], p.shape[1], p.shape[2]) if p.dim() == 4 else (0, 0, 0)
                    ok = p.dim() == 4 and p.is_contiguous() and k == p.shape[3] and k in (1, 3) and fw.numel() == n and fw.device == p.device \
                        and fw.dtype == torch.float32 and s64.dtype == torch.float64 and s64.numel() == O and s64.is_contiguous() \
                        and (fw.is_contiguous() if k == 1 else fw.permute(0, 2, 3, 1).is_contiguous())
                    if not ok:
                        raise AfiError(f"DetectorOptim: {self.names[i]} {tuple(p.shape)} / its folded weight {tuple(fw.shape)} are not a contiguous "
                                       "[O, I, k, k] weight (k 1 or 3) and its fold in the kernels' memory")
                    d.fold_out, d.s64, d.O, d.I, d.k = fw.data_ptr(), s64.data_ptr(), O, I, k
                    written.append(fw)
                    units.append(self._unit_count(i, n, O, I, k, True))
                else:
                    units.append(self._unit_count(i, n, 0, 0, 0, False))
            ops.detector_sgd_step(table, self.device, self.momentum, gscale, flat=self.FLAT_GRID, units=units)
            # a raw-pointer write bumps no version: do what torch's in-place update would have done, so every cache keyed on a parameter's
            # version (the RPN's, the heads') rebuilds, and a backward whose forward saved one of these tensors refuses to run
            torch.autograd.graph.increment_version([self.params[i] for i in live] + written)
            for net in self.modules:
                net.adopt_folded()
        self.iter += 1

    # ---- state
    def _logical(self, i):
        p = self.params[i]
        return torch.as_strided(self.flat_mom, p.size(), p.stride(), self._offs[i])

    def state_dict(self) -> Dict[str, object]:
        """Stage2Adversarial.state_dict's format: momentum buffers by parameter NAME in logical shape, the iteration, the schedule."""
        steps, gamma, wf, wi = self.sched
        mom = {n: self._logical(i).detach().clone(memory_format=torch.contiguous_format) for i, n in enumerate(self.names)}
        return {"iteration": int(self.iter), "optimizer": {"momentum_buffer": mom},
                "scheduler": {"last_epoch": int(self.iter), "base_lr": self.base_lr, "steps": list(steps), "gamma": gamma,
                              "warmup_factor": wf, "warmup_iters": wi}}

    def load_state_dict(self, sd: Dict[str, object]):
        """Inverse of ``state_dict``.  The schedule is a constructor argument: a stored one that differs is refused, not ignored."""
        sch = sd.get("scheduler")
        if sch is not None:
            mine = self.state_dict()["scheduler"]
            for k in ("base_lr", "steps", "gamma", "warmup_factor", "warmup_iters"):
                if k in sch and (list(sch[k]) != list(mine[k]) if k == "steps" else abs(float(sch[k]) - float(mine[k])) > 1e-12 * max(1.0, abs(float(mine[k])))):
                    raise ValueError(f"checkpoint scheduler {k} = {sch[k]!r} differs from this optimizer's {mine[k]!r}")
        mom = sd["optimizer"]["momentum_buffer"]
        missing, extra = [n for n in self.names if n not in mom], [n for n in mom if n not in set(self.names)]
        if missing or extra:
            raise KeyError(f"optimizer state: missing {missing}, unexpected {extra}")
        for i, n in enumerate(self.names):
            if tuple(mom[n].shape) != tuple(self.params[i].shape):
                raise ValueError(f"optimizer state {n}: shape {tuple(mom[n].shape)} != {tuple(self.params[i].shape)}")
            self._logical(i).copy_(mom[n].to(self.device, torch.float32))
        self.iter = int(sd["iteration"])


def build_detector_optimizer(cfg, model):
    """``build_optimizer(cfg, model)`` + ``build_lr_scheduler`` of detectron2 v0.1.1 as one DetectorOptim, from ``cfg.SOLVER`` (detectron2's
    defaults for absent keys)."""
    s = cfg_get(cfg, "SOLVER", None)
    if cfg_get(s, "NESTEROV", False):
        raise AfiError("SOLVER.NESTEROV is not supported (the step kernel is plain momentum SGD)")
    if cfg_get(cfg_get(s, "CLIP_GRADIENTS", None), "ENABLED", False):
        raise AfiError("SOLVER.CLIP_GRADIENTS.ENABLED is not supported (no gradient clipping in the step kernel)")
    sched = cfg_get(s, "LR_SCHEDULER_NAME", "WarmupMultiStepLR")
    if sched != "WarmupMultiStepLR":
        raise AfiError(f"SOLVER.LR_SCHEDULER_NAME {sched!r} is not supported (WarmupMultiStepLR only)")
    if cfg_get(s, "WARMUP_METHOD", "linear") != "linear":
        raise AfiError(f"SOLVER.WARMUP_METHOD {cfg_get(s, 'WARMUP_METHOD', 'linear')!r} is not supported (linear only)")
    return DetectorOptim(list(model.named_parameters()), base_lr=cfg_get(s, "BASE_LR", 0.001), momentum=cfg_get(s, "MOMENTUM", 0.9),
                         weight_decay=cfg_get(s, "WEIGHT_DECAY", 1e-4), weight_decay_norm=cfg_get(s, "WEIGHT_DECAY_NORM", 0.0),
                         bias_lr_factor=cfg_get(s, "BIAS_LR_FACTOR", 1.0), weight_decay_bias=cfg_get(s, "WEIGHT_DECAY_BIAS", 1e-4),
                         lr_steps=tuple(cfg_get(s, "STEPS", (30000,))), lr_gamma=cfg_get(s, "GAMMA", 0.1),
                         warmup_factor=cfg_get(s, "WARMUP_FACTOR", 1.0 / 1000), warmup_iters=cfg_get(s, "WARMUP_ITERS", 1000),
                         modules=list(model.modules()), norm_params=norm_module_params(model))


class DetectorStep:
    """detectron2's ``SimpleTrainer.run_step`` (engine/train_loop.py), the loop of the reference's ``Target_Detector_Trainer``:

        loss_dict = model(data); losses = sum(loss_dict.values()); optimizer.zero_grad(); losses.backward(); optimizer.step()

    `model` returns the loss dict in training mode (``GeneralizedRCNN``); a ``(loss_dict, extras)`` tuple (``GeneralizedRCNN_AFExtractor``) is
    accepted.  Data-parallel wrapping of `model` is the caller's, as in Stage2Step."""

    def __init__(self, model, optimizer):
        self.model, self.optimizer = model, optimizer
        self.iter = 0
        self.last_losses: Dict[str, float] = {}

    def run_step(self, data):
        if not self.model.training:
            raise AssertionError("[DetectorStep] model was changed to eval mode!")
        loss_dict = self.model(data)
        if isinstance(loss_dict, tuple):
            loss_dict = loss_dict[0]
        losses = sum(loss_dict.values())
        if not torch.isfinite(losses).all():
            raise FloatingPointError(f"Loss became infinite or NaN at iteration={self.iter}!\nloss_dict = {loss_dict}")
        self.optimizer.zero_grad()
        losses.backward()
        self.optimizer.step()
        self.iter += 1
        self.last_losses = {k: float(v.detach()) for k, v in loss_dict.items()}
        return self.last_losses


class GeneralizedRCNN(GeneralizedRCNN_AFExtractor):
    """detectron2's ``GeneralizedRCNN`` as step 3 trains it: ``GeneralizedRCNN_AFExtractor`` reading the full-size ``image`` and its
    ``instances`` (or ``targets``), and returning the loss dict alone in training.  Inference is the parent's, on ``image``."""

    def preprocess_image(self, batched_inputs):
        images = [(x["image"].to(self.device).float() - self.pixel_mean) / self.pixel_std for x in batched_inputs]
        sizes = [tuple(t.shape[-2:]) for t in images]
        return _Images(pad_to_batch(images, self.backbone.size_divisibility), sizes)

    def forward(self, batched_inputs):
        if not self.training:
            return self.inference(batched_inputs)
        images = self.preprocess_image(batched_inputs)
        if "instances" in batched_inputs[0]:
            gt_instances = [x["instances"].to(self.device) if hasattr(x["instances"], "to") else x["instances"] for x in batched_inputs]
        elif "targets" in batched_inputs[0]:
            gt_instances = [x["targets"] for x in batched_inputs]
        else:
            gt_instances = None
        features = self.backbone(images.tensor)
        if self.proposal_generator:
            proposals, proposal_losses = self.proposal_generator(images, features, gt_instances)
        else:
            assert "proposals" in batched_inputs[0]
            proposals = [x["proposals"] for x in batched_inputs]
            proposal_losses = {}
        _, detector_losses = self.roi_heads(images, features, proposals, gt_instances)
        losses = {}
        losses.update(detector_losses)
        losses.update(proposal_losses)
        return losses


def _detectron2_importable():
    try:
        import detectron2.modeling  # noqa: F401
        return True
    except Exception:
        return False


if not _detectron2_importable():                          # detectron2's own class owns the name in detectron2's registry
    META_ARCH_REGISTRY.register(GeneralizedRCNN)
