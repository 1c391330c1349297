"""The RSN pose refine machine (csrc/prm.hip): ``RSN_ATTENTION`` and ``RSN_WEIGHT_VECTOR``."""
from __future__ import annotations

import torch

from .. import hip
from .base import ACT_RELU, check_f32, require_gpu, _f32, _launch
from .conv import conv2d

PRM_MAX_CHANNELS = 64                 # what csrc/prm.hip takes (otp_prm_supported)


def check_prm(c, h, w):
    """Raise ``ValueError`` for a shape the PRM kernels do not take (``otp_prm_supported``: at most 64 channels)."""
    if min(c, h, w) < 1 or not hip.lib().otp_prm_supported(c, h, w):
        raise ValueError(f"prm: 1 <= channels <= {PRM_MAX_CHANNELS} on a non-empty plane, got {c} channels on {h} x {w}")


def fold_conv_bn(m, device):
    """(weight, scale, shift) of a ``modules.conv_bn_relu`` in eval mode: BatchNorm's running statistics as a per-channel scale and
    shift with the conv bias folded into the shift (what ``InferenceEngine._bn_fold`` computes)."""
    f = lambda t: _f32(t, device)                                                # noqa: E731
    sc = f(m.bn.weight) / torch.sqrt(f(m.bn.running_var) + m.bn.eps)
    sh = f(m.bn.bias) - f(m.bn.running_mean) * sc
    if m.conv.bias is not None:
        sh = sh + f(m.conv.bias) * sc
    return f(m.conv.weight), sc.contiguous(), sh.contiguous()


def _prm_layer(what, c, weight, scale, shift, taps, device):
    """The checked flat fp32 forms of one folded PRM layer: weight (C, taps), scale (C), shift (C)."""
    if weight.numel() != c * taps or scale.numel() != c or shift.numel() != c:
        raise ValueError(f"prm: {what} must hold ({c}, {taps}) weights and {c} scales and shifts, got {tuple(weight.shape)}, "
                         f"{tuple(scale.shape)}, {tuple(shift.shape)}")
    return _f32(weight, device).reshape(c, taps), _f32(scale, device).reshape(c), _f32(shift, device).reshape(c)


def prm_layer(layer, taps, device):
    """The folded (weight (C, taps), scale (C), shift (C)) of a gate layer (a ``modules.conv_bn_relu`` with C output channels)."""
    return _prm_layer(type(layer).__name__, layer.conv.out_channels, *fold_conv_bn(layer, device), taps, device)


def prm_gate_args(f, l1, l2, gate, residual):
    n, c, h, w = f.shape
    return (hip.ptr(f), *(hip.ptr(t) for t in l1), *(hip.ptr(t) for t in l2), hip.ptr(gate), n, c, h * w, int(bool(residual)))


def prm_apply_args(f, gate, l31, l32, out):
    n, c, h, w = f.shape
    return (hip.ptr(f), hip.ptr(gate), *(hip.ptr(t) for t in l31), *(hip.ptr(t) for t in l32), hip.ptr(out), n, c, h, w)


def prm_gate(f, w1, scale1, shift1, w2, scale2, shift2, residual=False):
    """The channel gate of RSN_ATTENTION / the tail of RSN_WEIGHT_VECTOR (RSB.py:160-164, 195-198) on f (N, C, H, W):
    ``sigmoid(relu(scale2 * (w2 @ v) + shift2))`` with ``v = relu(scale1 * (w1 @ mean_hw f) + shift1)`` (``+ mean_hw f`` with
    ``residual``) -> (N, C, 1, 1).  w (C, C[, 1, 1]); scale / shift (C): the folded BatchNorm and conv bias."""
    require_gpu(f, w1, w2)
    check_f32(f, w1, w2)
    if f.dim() != 4:
        raise ValueError(f"prm_gate: f must be (N, C, H, W), got {tuple(f.shape)}")
    f = f.contiguous()
    n, c, h, w = f.shape
    check_prm(c, h, w)
    l1 = _prm_layer("layer 1", c, w1, scale1, shift1, c, f.device)
    l2 = _prm_layer("layer 2", c, w2, scale2, shift2, c, f.device)
    gate = torch.empty((n, c, 1, 1), dtype=torch.float32, device=f.device)
    _launch(hip.lib().otp_prm_gate, "otp_prm_gate", prm_gate_args(f, l1, l2, gate, residual), f)
    return gate


def prm_apply(f, gate_c, w31, scale31, shift31, w32, scale32, shift32):
    """The spatial gate of RSN_ATTENTION and the output (RSB.py:199-202) as one launch: ``t = relu(scale31 * conv1x1(f, w31) +
    shift31)``, ``gate_s = sigmoid(relu(scale32 * dwconv9x9(t, w32, padding=4) + shift32))``, ``f * (1 + gate_c * gate_s)``.
    f (N, C, H, W), gate_c (N, C[, 1, 1]), w31 (C, C[, 1, 1]), w32 (C, 1, 9, 9)."""
    require_gpu(f, gate_c, w31, w32)
    check_f32(f, gate_c, w31, w32)
    if f.dim() != 4:
        raise ValueError(f"prm_apply: f must be (N, C, H, W), got {tuple(f.shape)}")
    f = f.contiguous()
    n, c, h, w = f.shape
    check_prm(c, h, w)
    if gate_c.numel() != n * c:
        raise ValueError(f"prm_apply: gate_c must hold ({n}, {c}) entries, got {tuple(gate_c.shape)}")
    l31 = _prm_layer("layer 3_1", c, w31, scale31, shift31, c, f.device)
    l32 = _prm_layer("layer 3_2", c, w32, scale32, shift32, 81, f.device)
    out = torch.empty_like(f)
    _launch(hip.lib().otp_prm_apply, "otp_prm_apply", prm_apply_args(f, gate_c.contiguous(), l31, l32, out), f)
    return out


def _prm_front(x, m, what):
    """``relu(bn(conv3x3(x)))`` of the module's first layer on the exact-fp32 direct convolution."""
    require_gpu(x)
    check_f32(x)
    if m.training:
        raise RuntimeError(f"ops.{what} is the eval path (folded BatchNorm); train through otpose_amd.train.TrainGraph")
    if x.dim() != 4 or x.shape[1] != m.conv.in_channels:
        raise ValueError(f"{what}: x must be (N, {m.conv.in_channels}, H, W), got {tuple(x.shape)}")
    check_prm(m.conv.out_channels, x.shape[2], x.shape[3])
    w, sc, sh = fold_conv_bn(m, x.device)
    return conv2d(x, w, sc, sh, 1, 1, 1, ACT_RELU)


def rsn_attention(x, module):
    """``modules.RSN_ATTENTION`` in eval mode (RSB.py:192-203) on x (N, C, H, W): the 3x3 layer, :func:`prm_gate`, :func:`prm_apply`."""
    f = _prm_front(x, module.conv_bn_relu_prm_1, "rsn_attention")
    dev = x.device
    gate = prm_gate(f, *fold_conv_bn(module.conv_bn_relu_prm_2_1, dev), *fold_conv_bn(module.conv_bn_relu_prm_2_2, dev))
    return prm_apply(f, gate, *fold_conv_bn(module.conv_bn_relu_prm_3_1, dev), *fold_conv_bn(module.conv_bn_relu_prm_3_2, dev))


def rsn_weight_vector(x, module):
    """``modules.RSN_WEIGHT_VECTOR`` in eval mode (RSB.py:158-165) on x (N, Cin, H, W) -> (N, C, 1, 1): the 3x3 layer, then
    :func:`prm_gate` with the inner residual."""
    f = _prm_front(x, module.conv_bn_relu_1, "rsn_weight_vector")
    dev = x.device
    return prm_gate(f, *fold_conv_bn(module.conv_bn_relu_2, dev), *fold_conv_bn(module.conv_bn_relu_3, dev), residual=True)
