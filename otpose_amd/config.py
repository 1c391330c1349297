"""Configuration node + built-in OTPose configurations.

The reference reads its configuration through a yacs ``CfgNode`` that is accessed both as
attributes (``cfg.MODEL.NUM_JOINTS``, reference model/OTPose.py:191-199) and as a mapping
(``cfg['MODEL']['EXTRA']``, reference model/OTPose.py:185,223; model/HRNet.py:75).  yacs is not
part of this image, so :class:`CfgNode` below is a minimal stand-in with the same two access
styles plus the ``_BASE_`` yaml inheritance of reference utils/setup.py:54-69.

Only the keys the hot path reads are given defaults ("Config / flags"):
``MODEL.{NUM_JOINTS,HEATMAP_SIZE,IMAGE_SIZE,PRETRAINED,FREEZE_HRNET_WEIGHTS,DEFORMABLE_CONV.*,
DEFORMABLE_CONV_CH,OFFSET_MASK_COMBINE_CONV,EXTRA.*}`` and ``LOSS.{NAME,USE_TARGET_WEIGHT}``.
Values follow reference configs/Base_PoseTrack17.yaml:36-88 and configs/17/model_RSN.yaml:28-40.

Extension keys read with a default when absent (``otpose_amd.model.OTPose``): ``MODEL.WINDOW_FRAMES``, ``MODEL.DTYPE`` and the
local attention windows ``MODEL.MHA_WIN_SIZE`` (int or per-level list, -1 = off), ``MODEL.USE_REL_PE`` (False) for the two temporal
encoders and ``MODEL.FLOW_MHA_WIN_SIZE`` (-1) for the flow encoder; the conv embedding layers in front of the encoders
(reference model/ConvVideoTransformer.py:60-78, ``arch[0]``): ``MODEL.EMBD_LAYERS`` (int, 0 = none) for the two temporal encoders,
``MODEL.FLOW_EMBD_LAYERS`` (0) for the flow encoder, ``MODEL.EMBD_KS`` (3; 1, 3 or 5) and ``MODEL.EMBD_WITH_LN`` (True: a channel
LayerNorm behind each convolution and no conv bias).  Training takes ``EMBD_KS`` 1 or 3.  ``MODEL.PRM`` (a tuple out of
``("def_fuse", "offset_mask_combine_conv")``, default ``()``): the output of a named RSB chain passes through an ``RSN_ATTENTION`` of
its channel count (reference model/RSB.py:168-203, RSN's Pose Refine Machine), held as ``def_fuse_prm`` /
``offset_mask_combine_prm``.  The reference exports that class and has no call site for it: the placement is this package's.
The token encoders (reference model/OTPose.py:26-159, the DETR-style ``TransformerEncoder`` it exports and never calls):
``MODEL.TOKEN_LAYERS`` (int, 0 = none) puts one of that many layers in front of each temporal encoder (``token_encoder1`` /
``token_encoder2``, over the h w tokens of width 8 J), ``MODEL.FLOW_TOKEN_LAYERS`` (0) in front of the flow encoder
(``flow_token_encoder``, width J, one head, FFN 2 J); ``MODEL.TOKEN_HEADS`` (2; divides the width, heads of at most 136 channels),
``MODEL.TOKEN_FFN`` (2 x the width), ``MODEL.TOKEN_PRE_NORM`` (False), ``MODEL.TOKEN_PE`` (``"sine"``, ``"learnable"`` or
``"none"``: the tables ``temporal_pos_embedding`` / ``flow_pos_embedding`` of OTPose.py:259-279; with ``"sine"`` the flow encoder
runs without a table, width J = 17 has none), ``MODEL.TOKEN_PRODUCTS`` (``"f32"`` or ``"half"``: the attention products of all
three token encoders in exact fp32, or with IEEE-half operands and fp32 accumulation, csrc/tokattn_h.hip).  A malformed value raises ``ValueError`` also when no layer is asked for.
Attention-probability dropout, training only (reference model/blocks.py:392,572 and the ``dropout`` OTPose.py:93 hands to
``nn.MultiheadAttention``; its OTPose.py:209-216 leaves the rate at 0): ``MODEL.ATTN_PDROP`` (0.0) for the two temporal encoders,
``MODEL.FLOW_ATTN_PDROP`` (0.0) for the flow encoder, ``MODEL.TOKEN_ATTN_DROPOUT`` (0.0) for the token encoders; floats in [0, 1).
The training graph applies the first two to the channel attention; together with local windows for the same encoder they raise ``ValueError``.
"""
from __future__ import annotations

import copy
import os
from typing import Any, Dict, Iterable, Tuple


class CfgNode(dict):
    """dict with attribute access, recursively applied to nested mappings."""

    def __init__(self, init: Dict[str, Any] | None = None):
        super().__init__()
        for k, v in (init or {}).items():
            self[k] = v

    @staticmethod
    def _wrap(v):
        if isinstance(v, dict) and not isinstance(v, CfgNode):
            return CfgNode(v)
        if isinstance(v, tuple):
            return list(v)
        return v

    def __setitem__(self, k, v):
        super().__setitem__(k, self._wrap(v))

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def merge(self, other: Dict[str, Any]) -> "CfgNode":
        """Recursive in-place merge (``other`` wins)."""
        for k, v in other.items():
            if isinstance(v, dict) and isinstance(self.get(k), dict):
                self[k].merge(v)
            else:
                self[k] = copy.deepcopy(v)
        return self

    def clone(self) -> "CfgNode":
        return CfgNode(copy.deepcopy(dict(self)))


def load_yaml(path: str) -> CfgNode:
    """Load a yaml experiment file, following a ``_BASE_`` chain relative to the file."""
    import yaml

    with open(path, "r") as f:
        raw = yaml.safe_load(f) or {}
    base = raw.pop("_BASE_", None)
    if base is not None:
        cfg = load_yaml(os.path.join(os.path.dirname(path), base))
        cfg.merge(raw)
        return cfg
    return CfgNode(raw)


def _stage(modules: int, channels: Iterable[int]) -> Dict[str, Any]:
    channels = list(channels)
    return {
        "NUM_MODULES": modules,
        "NUM_BRANCHES": len(channels),
        "BLOCK": "BASIC",
        "NUM_BLOCKS": [4] * len(channels),
        "NUM_CHANNELS": channels,
        "FUSE_METHOD": "SUM",
    }


def make_cfg(width: int = 48, image_size: Tuple[int, int] = (288, 384),
             dilations: Iterable[int] = (3, 6, 9, 12, 15), frames: int = 5, dtype: str = "fp32") -> CfgNode:
    """Built-in OTPose configuration.

    ``frames`` = frames per clip window: 5 is the reference (hard-coded at model/OTPose.py:309,320-321); 7 is this build's
    extension for BASELINE configs[4] (``MODEL.WINDOW_FRAMES``, 12 stacked maps per joint: oracle ``window_maps``).

    ``dtype`` = ``MODEL.DTYPE`` of the EVAL forward: "fp32" (the reference's arithmetic) or "fp16" (BASELINE configs[4]: backbone
    activations stored as IEEE half, one f16 MFMA per product - otpose_amd/engine_h16.py; an extension, never a default).

    ``width`` is the HRNet branch-0 width (48 = the reference's W48 yaml, 32 = HRNet-W32 used by
    BASELINE.json configs[0]); ``image_size`` is (W, H) as in the reference yaml.
    """
    w, h = image_size
    assert w % 32 == 0 and h % 32 == 0, "image size must be divisible by 32 (four HRNet branches)"
    c = [width, 2 * width, 4 * width, 8 * width]
    return CfgNode({
        "MODEL": {
            "NAME": "OTPose",
            "NUM_JOINTS": 17,
            "WINDOW_FRAMES": int(frames),
            "DTYPE": str(dtype),
            "IMAGE_SIZE": [w, h],
            "HEATMAP_SIZE": [w // 4, h // 4],
            "PRETRAINED": "",
            "FREEZE_HRNET_WEIGHTS": False,
            "DEFORMABLE_CONV_CH": 32,
            "OFFSET_MASK_COMBINE_CONV": 2,
            "DEFORMABLE_CONV": {"DILATION": list(dilations), "AGGREGATION_TYPE": "weighted_sum"},
            "EXTRA": {
                "PRETRAINED_LAYERS": ["*"],
                "FINAL_CONV_KERNEL": 1,
                "STAGE2": _stage(1, c[:2]),
                "STAGE3": _stage(4, c[:3]),
                "STAGE4": _stage(3, c[:4]),
            },
        },
        "LOSS": {"NAME": "ST_OHKW_MSELoss", "USE_TARGET_WEIGHT": True, "TOPK": 8},
        # optimizer / schedule keys read by optim.make_optimizer and schedule.make_scheduler: reference configs/default.py:136-160
        # overridden by configs/Base_PoseTrack17.yaml:106-120
        "TRAIN": {"LR": 1e-4, "WD": 0.0, "OPTIMIZER": "AdamW", "MOMENTUM": 0.9, "NESTEROV": False,
                  "LR_SCHEDULER": "CosineAnnealingLR", "WARMUP": True, "WARMUP_EPOCHS": 12, "END_EPOCH": 38, "EPOCHS": 30,
                  "GAMMA": 0.9},
    })


def cfg1() -> CfgNode:
    """BASELINE.json configs[0]: 256x192 clip, HRNet-W32."""
    return make_cfg(32, (192, 256))


def cfg2() -> CfgNode:
    """BASELINE.json configs[1]: 384x288 clip, HRNet-W48 (the metric's configuration)."""
    return make_cfg(48, (288, 384))


def tiny_cfg(width: int = 8, image_size: Tuple[int, int] = (64, 96), frames: int = 5, dtype: str = "fp32") -> CfgNode:
    """A reduced-width, reduced-resolution model with the full OTPose topology (test sizes)."""
    return make_cfg(width, image_size, frames=frames, dtype=dtype)


def cfg5(dtype: str = "fp32") -> CfgNode:
    """BASELINE.json configs[4]: 7-frame window at 384x288 (extension; the reference has no such model); ``dtype="fp16"`` is the
    configuration as BASELINE.json states it."""
    return make_cfg(48, (288, 384), frames=7, dtype=dtype)
