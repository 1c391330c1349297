"""otpose_amd - MI355X-native (gfx950) implementation of the OTPose hot path.

Public surface (mirrors the reference's module / operator API for the path in SURVEY.md section 8):
``OTPose`` (model/OTPose.py), ``ModulatedDeformConv`` / ``DeformableCONV`` /
``modulated_deform_conv`` and the deformable RoI pooling (thirdparty/deform_conv), the heatmap losses (model/loss.py), the
training set-up ``make_optimizer`` / ``make_scheduler`` / ``ModelEma`` (thirdparty/utils/train_utils.py:62-262), the person
detector ``PersonDetector`` (object_detector/YOLOv3), the fixed-batch video driver ``VideoPose`` and the
1-process-per-GPU data-parallel helpers (replacing nn.DataParallel, train.py:78-79).
"""
from .config import CfgNode, cfg1, cfg2, make_cfg, tiny_cfg, load_yaml  # noqa: F401
from .model import OTPose, ModulatedDeformConv, DeformableCONV  # noqa: F401
from .ops import modulated_deform_conv  # noqa: F401
from .deform_pool import (DeformRoIPoolingFunction, deform_roi_pooling, DeformRoIPooling, DeformRoIPoolingPack,  # noqa: F401
                          ModulatedDeformRoIPoolingPack)
from .optim import FusedAdamW, FusedSGD, make_optimizer  # noqa: F401
from .ema import ModelEma  # noqa: F401
from .schedule import LinearWarmupCosineAnnealingLR, LinearWarmupMultiStepLR, make_scheduler  # noqa: F401
from .detector import PersonDetector, parse_darknet_cfg, yolov3_defs  # noqa: F401
from .video import VideoPose  # noqa: F401
from . import parallel  # noqa: F401  (installs the process-group hooks: parallel.graph_replay_safe)

__all__ = ["OTPose", "ModulatedDeformConv", "DeformableCONV", "modulated_deform_conv",
           "DeformRoIPoolingFunction", "deform_roi_pooling", "DeformRoIPooling", "DeformRoIPoolingPack",
           "ModulatedDeformRoIPoolingPack",
           "make_optimizer", "make_scheduler", "ModelEma", "FusedAdamW", "FusedSGD", "LinearWarmupCosineAnnealingLR",
           "LinearWarmupMultiStepLR", "PersonDetector", "parse_darknet_cfg", "yolov3_defs", "VideoPose",
           "CfgNode", "make_cfg", "cfg1", "cfg2", "tiny_cfg", "load_yaml"]
