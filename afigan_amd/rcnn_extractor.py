"""``GeneralizedRCNN_AFExtractor`` (afigan/modeling/meta_arch/rcnn_extractor.py:21-147): the stage-2 detector, a GeneralizedRCNN that runs on
``image_x0.5`` and ALSO hands back its FPN features, which the stage-2 loop trains against the guide network's.

The backbone is the AFI pyramid of this package (FPN_AFIGAN / PAFPN_AFIGAN through BACKBONE_REGISTRY); the proposal generator is
detectron2's when it is importable and this package's frozen, inference-only ``rpn.RPN`` otherwise; the ROI heads are built from a config
by detectron2 when it is importable, and the constructor takes any callables with their contracts otherwise: ``roi_heads=`` this package's
frozen box branch (``afigan_amd.build_roi_heads(cfg, backbone.output_shape())``, roi_heads.py; ``masks=True`` adds the mask branch, whose
``pred_masks`` the postprocess pastes into image-size bool masks), or a stand-in."""
import torch
import torch.nn as nn

from .rcnn_only import pad_to_batch
from .registry import BACKBONE_REGISTRY, Registry

try:                                                     # the reference registers into detectron2's META_ARCH_REGISTRY (:21)
    from detectron2.modeling import META_ARCH_REGISTRY
except Exception:
    META_ARCH_REGISTRY = Registry("META_ARCH")


class _Images:
    """What detectron2's ImageList gives the heads: the padded batch and the un-padded sizes."""

    def __init__(self, tensor, image_sizes):
        self.tensor, self.image_sizes = tensor, image_sizes

    def __len__(self):
        return len(self.image_sizes)


@META_ARCH_REGISTRY.register()
class GeneralizedRCNN_AFExtractor(nn.Module):
    def __init__(self, cfg=None, *, backbone=None, proposal_generator=None, roi_heads=None, pixel_mean=None, pixel_std=None,
                 device=None, input_format="BGR"):
        super().__init__()
        if cfg is not None and backbone is None:
            built = self._build_from_config(cfg)
            backbone, proposal_generator, roi_heads = built
            pixel_mean, pixel_std, device, input_format = cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD, cfg.MODEL.DEVICE, cfg.INPUT.FORMAT
        self.device = torch.device(device if device is not None else "cuda")
        self.backbone, self.proposal_generator, self.roi_heads = backbone, proposal_generator, roi_heads
        self.input_format = input_format
        assert len(pixel_mean) == len(pixel_std)
        n = len(pixel_mean)
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean, dtype=torch.float32).view(n, 1, 1), persistent=False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std, dtype=torch.float32).view(n, 1, 1), persistent=False)
        self.to(self.device)

    @staticmethod
    def _build_from_config(cfg):
        """rcnn_extractor.py:27-29,134-147: backbone from BACKBONE_REGISTRY, RPN / ROI heads from detectron2."""
        from .fpn_sr import ShapeSpec
        backbone = BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, ShapeSpec(channels=len(cfg.MODEL.PIXEL_MEAN), stride=None))
        try:
            from detectron2.modeling.proposal_generator import build_proposal_generator
        except Exception:
            from .rpn import build_proposal_generator                  # this package's RPN (frozen until RPN.trainable_(); losses: DESIGN 21)
        proposal_generator = build_proposal_generator(cfg, backbone.output_shape())
        try:
            from detectron2.modeling.roi_heads import build_roi_heads
        except Exception as e:
            from ._lib import AfiError
            raise AfiError(f"building the ROI heads from a config needs detectron2 ({type(e).__name__}: {e}); "
                           "pass proposal_generator= and roi_heads= instead")
        return backbone, proposal_generator, build_roi_heads(cfg, backbone.output_shape())

    def preprocess_image(self, batched_inputs):
        """rcnn_extractor.py:120-127: the detector sees the HALF-size image of the dual-scale mapper."""
        images = [(x["image_x0.5"].to(self.device).float() - self.pixel_mean) / self.pixel_std for x in batched_inputs]
        sizes = [tuple(t.shape[-2:]) for t in images]
        return _Images(pad_to_batch(images, self.backbone.size_divisibility), sizes)

    def forward(self, batched_inputs, img_dict_name="image"):
        if not self.training:
            return self.inference(batched_inputs)
        images = self.preprocess_image(batched_inputs)
        if "instances" in batched_inputs[0]:                                           # :45-50 (the x0.5 annotations)
            gt_instances = [x["instances_x0.5"].to(self.device) if hasattr(x["instances_x0.5"], "to") else x["instances_x0.5"] for x in batched_inputs]
        elif "targets" in batched_inputs[0]:
            gt_instances = [x["targets"] for x in batched_inputs]
        else:
            gt_instances = None
        features = self.backbone(images.tensor)                                        # :53
        processed_results = [{"features": features}]                                   # :55-56
        if self.proposal_generator:
            proposals, proposal_losses = self.proposal_generator(images, features, gt_instances)    # :58-59
        else:
            assert "proposals" in batched_inputs[0]
            proposals = [x["proposals"] for x in batched_inputs]
            proposal_losses = {}
        _, detector_losses = self.roi_heads(images, features, proposals, gt_instances)           # :65
        losses = {}
        losses.update(detector_losses)
        losses.update(proposal_losses)
        return losses, processed_results                                               # :67-70

    def inference(self, batched_inputs, detected_instances=None, do_postprocess=True, mask_format="bitmask"):
        """rcnn_extractor.py:72-118: features -> proposals -> ROI-head predictions, then (do_postprocess) each image's instances rescaled
        to the input's "height" / "width" and wrapped as ``{"instances": r}`` -- the contract evaluators are written against.
        mask_format "rle": the postprocess is this package's own, and the instances carry ``pred_masks_rle`` (a list of COCO RLE dicts at
        the output size, roi_heads.paste_masks_rle) instead of the image-size bool ``pred_masks``, which are never formed."""
        assert not self.training
        if mask_format not in ("bitmask", "rle"):
            from ._lib import AfiError
            raise AfiError(f"inference: mask_format must be 'bitmask' or 'rle', got {mask_format!r}")
        images = self.preprocess_image(batched_inputs)
        features = self.backbone(images.tensor)
        if detected_instances is None:
            if self.proposal_generator:
                proposals, _ = self.proposal_generator(images, features, None)
            else:
                assert "proposals" in batched_inputs[0]
                proposals = [x["proposals"].to(self.device) if hasattr(x["proposals"], "to") else x["proposals"] for x in batched_inputs]
            results, _ = self.roi_heads(images, features, proposals, None)
        else:
            detected_instances = [x.to(self.device) if hasattr(x, "to") else x for x in detected_instances]        # :101
            results = self.roi_heads.forward_with_given_boxes(features, detected_instances)
        if do_postprocess:
            return self._postprocess(results, batched_inputs, images.image_sizes, mask_format)                      # :106-107
        return results

    @staticmethod
    def _postprocess(instances, batched_inputs, image_sizes, mask_format="bitmask"):
        """rcnn_extractor.py:129-143: ``detector_postprocess(results, height, width)`` per image.  detectron2's own function when it is
        importable; otherwise its box part (scale by output / network size, clip, drop empty boxes: detectron2 v0.1.1
        modeling/postprocessing.py) on anything that carries ``image_size`` and ``pred_boxes``, then ``pred_masks`` pasted at the output
        size into the scaled boxes (roi_heads.paste_masks_in_image, GPU only) -- and a loud error for the instance field this package cannot
        rescale without detectron2 (keypoints) rather than a silently wrong scale."""
        if mask_format == "rle":                        # detectron2's function knows only the bitmask
            def detector_postprocess(r, h, w):
                return _detector_postprocess_boxes(r, h, w, mask_format="rle")
        else:
            try:
                from detectron2.modeling.postprocessing import detector_postprocess
            except Exception:
                detector_postprocess = _detector_postprocess_boxes
        out = []
        for results_per_image, input_per_image, image_size in zip(instances, batched_inputs, image_sizes):
            height = input_per_image.get("height", image_size[0])
            width = input_per_image.get("width", image_size[1])
            out.append({"instances": detector_postprocess(results_per_image, height, width)})
        return out


def _detector_postprocess_boxes(results, output_height, output_width, mask_format="bitmask"):
    import copy
    from ._lib import AfiError
    if mask_format not in ("bitmask", "rle"):
        raise AfiError(f"mask_format must be 'bitmask' or 'rle', got {mask_format!r}")
    if getattr(results, "pred_keypoints", None) is not None:
        raise AfiError("rescaling `pred_keypoints` to the input size needs detectron2's detector_postprocess (not importable here); "
                       "call inference(..., do_postprocess=False) for raw ROI-head results")
    masks = getattr(results, "pred_masks", None)
    if masks is not None and not getattr(masks, "is_cuda", False):
        raise AfiError("pasting `pred_masks` into the image runs on the GPU only (got a CPU tensor); there is no CPU fallback: call "
                       "inference(..., do_postprocess=False) for raw ROI-head results")
    h, w = results.image_size
    sx, sy = output_width / w, output_height / h
    # detectron2's Instances (reached under mask_format "rle" only): image_size is read-only and every field has one length, so the result is
    # a new object that receives the kept rows of every field; anything else is shallow-copied, as before
    inst = hasattr(results, "get_fields") and hasattr(results, "_image_size")
    if inst:
        r = type(results)((output_height, output_width))
    else:
        r = copy.copy(results)
        r.image_size = (output_height, output_width)
    boxes = getattr(results, "pred_boxes", None)
    if boxes is None:
        boxes = getattr(results, "proposal_boxes", None)
        name = "proposal_boxes"
    else:
        name = "pred_boxes"
    if boxes is None:
        if masks is not None:
            raise AfiError("`pred_masks` without `pred_boxes` to paste them into")
        if inst:
            for f, v in results.get_fields().items():
                r.set(f, v)
        return r
    t = (boxes.tensor if hasattr(boxes, "tensor") else boxes).clone()
    t[:, 0::2] *= sx
    t[:, 1::2] *= sy
    t[:, 0::2].clamp_(min=0, max=output_width)
    t[:, 1::2].clamp_(min=0, max=output_height)
    keep = ((t[:, 2] - t[:, 0]) > 0) & ((t[:, 3] - t[:, 1]) > 0)
    if hasattr(boxes, "tensor"):
        nb = copy.copy(boxes)
        nb.tensor = t[keep]
        setattr(r, name, nb)
    else:
        setattr(r, name, t[keep])
    if inst:
        for f, v in results.get_fields().items():
            if f not in (name, "pred_masks"):
                r.set(f, v[keep])
    else:
        for f in ("scores", "pred_classes", "objectness_logits"):
            v = getattr(results, f, None)
            if v is not None and hasattr(v, "__getitem__") and len(v) == len(keep):
                setattr(r, f, v[keep])
    if masks is not None:
        if name != "pred_boxes" or len(masks) != len(keep):
            raise AfiError(f"`pred_masks` of {len(masks)} rows without as many `pred_boxes` to paste them into")
        from .roi_heads import paste_masks_in_image, paste_masks_rle
        if mask_format == "rle":
            r.pred_masks_rle = paste_masks_rle(masks[keep], t[keep], (int(output_height), int(output_width)), threshold=0.5)
            if not inst:
                r.pred_masks = None
        else:
            r.pred_masks = paste_masks_in_image(masks[keep], t[keep], (int(output_height), int(output_width)), threshold=0.5)
    return r
