"""Operator-level Python API over the C-ABI (mirror of the reference's native operator boundary): one module per kernel
family, every public name re-exported here (``from otpose_amd import ops; ops.conv2d_x3(...)``).

    base       constants, device / dtype / shape checks, ``View`` / ``H8``, launch helpers (imports ``hip`` alone)
    dcn        the ``deform_conv_cuda`` drop-in names and autograd Functions, the fused warping head
    psroi      deformable PS-RoI pooling
    conv       fp32, Winograd, small, split-product, S8, stride-2, stem and pointwise convolutions, upsample-add
    encoder    temporal-encoder operators: LN + MLP, dense, q/k/v front, attention, conv embedding, flow-encoder blocks
    prm        the RSN pose refine machine
    h16        the H8 / fp16 record operators
    decode     heat-map decode, flip merge, PCK
    poseval    PoseTrack assignment, AP, pose NMS
    data       frame, crop, target and plan data preparation
    loss       the three losses
    detect     the YOLO detector passes
    segments   segment NMS and segment AP

Imports go one way: every module imports ``base``; ``prm`` and ``h16`` also import ``conv``; nothing imports this file.
"""
from .. import hip  # noqa: F401    (``ops.hip``: the binding the wrappers launch through, as ops.py had it)
from .base import (  # noqa: F401
    require_gpu, check_f32, out_hw, ACT_NONE, ACT_RELU, ACT_GELU, View, H8)
from .dcn import (  # noqa: F401
    modulated_deform_conv_cuda_forward, modulated_deform_conv_cuda_backward, ModulatedDeformConvFunction,
    modulated_deform_conv, deform_conv_forward_cuda, deform_conv_backward_input_cuda, deform_conv_backward_parameters_cuda,
    DeformConvFunction, deform_conv, dcn_fused_supported, pack_dcn_fused, dcn_fused)
from .psroi import (  # noqa: F401
    deform_psroi_pooling_cuda_forward, deform_psroi_pooling_cuda_backward)
from .conv import (  # noqa: F401
    pack_conv_weight, conv_desc, conv2d_args, conv2d_launch, pack_wino_weight, small_conv_supported, pack_small_conv_weight,
    conv3x3_small_args, conv3x3_small, h16_weight_exponent, x3_weight_exponent, pack_x3_weight, x3_supported, conv2d_x3_args,
    conv2d_x3_launch, conv2d_x3, S8_F32_C4, S8_F32_NCHW, s8_empty, c4_empty, s8_pack, s8_unpack, c4_unpack,
    s8_conv_supported, s8_conv_desc, s8_s2_conv_desc, s8_s2_conv_supported, conv3x3_s2_s8_args, conv3x3_s2_s8,
    pack_s8_weight, conv3x3_s8_args, conv3x3_s8_launch, conv3x3_s8, stem_conv_x3_supported, pack_stem_conv_x3,
    stem_conv_x3_args, stem_conv_x3, pointwise_x3_supported, pack_pointwise_x3, pointwise_x3_args, pointwise_x3,
    pointwise_x3_s8_supported, pack_pointwise_x3_s8, pointwise_x3_s8_res_args, pointwise_x3_s8, pointwise_x3_pair_supported,
    pack_pointwise_x3_pair, pointwise_x3_pair_args, pointwise_x3_pair, wino_supported, winograd_pays, runs_winograd,
    conv2d_wino_args, conv2d_wino_launch, conv2d_wino, conv2d, upsample_add_args, upsample_add, upsample_add_multi_args,
    upsample_add_multi)
from .encoder import (  # noqa: F401
    ln_mlp_args, ln_mlp_fused, dense_cc_supported, dense_x3_supported, pack_dense_cc, dense_cc_args, dense_cc,
    pack_qkv_table, qkv_front_args, qkv_front, mlp_fused_supported, pack_mlp_weights, mlp_fused, mlp_x3_supported,
    pack_mlp_x3_weights, mlp_x3, ln_mlp_x3, ln_channel, dwconv_ln3, chan_attn_args, chan_attn, check_local_attn,
    local_attn_args, rel_pe_table, local_attn, CONV_EMBD_KS, CONV_EMBD_MAX_CHANNELS, check_conv_embd, pack_conv_embd_weight,
    conv_embd_params, conv_embd_args, conv_embd, upsample_linear_args, upsample_linear, flow_block_supported,
    pack_flow_front, pack_flow_back, flow_front_args, flow_back_args, flow_front, flow_back)
from .prm import (  # noqa: F401
    PRM_MAX_CHANNELS, check_prm, fold_conv_bn, prm_layer, prm_gate_args, prm_apply_args, prm_gate, prm_apply, rsn_attention,
    rsn_weight_vector)
from .h16 import (  # noqa: F401
    h8_empty, h8_pack, h8_unpack, h16_conv_desc, h16_conv_supported, pack_h16_conv_weight, h16_conv3x3_args, h16_conv3x3,
    h16_pointwise_supported, pack_h16_pointwise, h16_pointwise_args, h16_pointwise, pack_h16_stem, h16_stem,
    h16_upsample_add_args, h16_upsample_add)
from .decode import (  # noqa: F401
    FLIP_PAIRS, get_max_preds, get_final_preds, flip_permutation, flip_test_merge, mirror_pair, accuracy)
from .poseval import (  # noqa: F401
    POSEVAL_JOINTS, POSEVAL_MAX_PR, POSEVAL_MAX_GT, pose_assign, sort_entries, ap_curve, COCO_SIGMAS, pose_nms)
from .data import (  # noqa: F401
    IMAGENET_MEAN, IMAGENET_STD, frames_to_clip, crop_clips, pose_targets, PosePlan, pose_plan)
from .loss import (  # noqa: F401
    st_ohkw_loss, joints_mse, joints_ohkm_mse_loss, joint_mse_loss)
from .detect import (  # noqa: F401
    letterbox, leaky_pass_args, leaky_pass, yolo_decode_args, yolo_decode, frame_rescale, box_nms_merge)
from .segments import (  # noqa: F401
    seg_nms, seg_softnms, seg_voting_groups, seg_ap_match, seg_ap)
