"""Deformable convolution (csrc/mdcn.hip, csrc/dcn_fused.hip): the reference's native operator boundary.

``modulated_deform_conv`` replaces ``thirdparty.deform_conv.modulated_deform_conv``
(reference thirdparty/deform_conv/functions/deform_conv.py:109-179): same argument order, same
``NotImplementedError`` for CPU tensors (functions/deform_conv.py:131,149), same gradient tuple.
``modulated_deform_conv_cuda_forward`` / ``_backward`` keep the pybind entry points' names and
argument lists (reference thirdparty/deform_conv/src/deform_conv_cuda.cpp:474-480, 551-558) for
callers that bind the native module directly.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd import Function

from .. import hip
from .base import _DTYPES, check_f32, out_hw, require_gpu, _f32, _image


def _dcn_dtype(*tensors):
    """Storage type code of a DCN call: every tensor must share one of the types the operator is instantiated for
    (the reference dispatches double / float / half, deform_conv_cuda_kernel.cu:719,751,784; bf16 is an addition)."""
    ts = [t for t in tensors if t is not None]
    dt = ts[0].dtype
    if dt not in _DTYPES:
        raise RuntimeError(f"deformable convolution is not implemented for {dt}")
    for t in ts:
        if t.dtype != dt:
            raise RuntimeError(f"deformable convolution: mixed dtypes {dt} / {t.dtype}")
    return _DTYPES[dt]


def modulated_deform_conv_cuda_forward(input, weight, bias, ones, offset, mask, output, columns,
                                       kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                                       dilation_h, dilation_w, group, deformable_group, with_bias):
    """In-place forward with the reference pybind signature (deform_conv_cuda.cpp:474-480).
    ``ones`` and ``columns`` are accepted and ignored: the fused kernel needs no im2col scratch.
    ``mask = None`` runs DCN v1 (no modulation) on the same kernels."""
    require_gpu(input, weight, offset, mask, output)
    b = bias if with_bias else None
    dtype = _dcn_dtype(input, weight, offset, mask, output, b)
    if not input.is_contiguous():
        raise RuntimeError("input tensor has to be contiguous")
    if not weight.is_contiguous():
        raise RuntimeError("weight tensor has to be contiguous")
    n, c, h, w = input.shape
    cout, cpg, kh_, kw_ = weight.shape
    if (kh_, kw_) != (kernel_h, kernel_w):
        raise RuntimeError(f"Input shape and kernel shape wont match: ({kernel_h} x {kernel_w} vs {kh_} x {kw_}).")
    if c != cpg * group:
        raise RuntimeError(f"Input shape and kernel channels wont match: ({c} vs {cpg * group}).")
    offset = offset.contiguous()
    mask = mask.contiguous() if mask is not None else None
    st = hip.lib().otp_mdcn_forward_ex(
        hip.ptr(input), hip.ptr(offset), hip.ptr(mask), hip.ptr(weight), hip.ptr(b), hip.ptr(output),
        n, c, h, w, cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
        deformable_group, 1.0, 0.0, dtype, hip.stream_of(input))
    hip.check(st, "otp_mdcn_forward")


def modulated_deform_conv_cuda_backward(input, weight, bias, ones, offset, mask, columns,
                                        grad_input, grad_weight, grad_bias, grad_offset, grad_mask,
                                        grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h,
                                        pad_w, dilation_h, dilation_w, group, deformable_group, with_bias):
    """In-place backward with the reference pybind signature (deform_conv_cuda.cpp:551-558).
    grad_input/grad_offset/grad_mask are overwritten; grad_weight/grad_bias are accumulated into
    (the reference accumulates them over the batch with addmm_, cpp:638-650).  ``mask = grad_mask = None``: DCN v1."""
    require_gpu(input, weight, offset, mask, grad_output)
    gb = grad_bias if with_bias else None
    dtype = _dcn_dtype(input, weight, offset, mask, grad_output, grad_input, grad_weight, grad_offset, grad_mask, gb)
    if not input.is_contiguous():
        raise RuntimeError("input tensor has to be contiguous")
    if not weight.is_contiguous():
        raise RuntimeError("weight tensor has to be contiguous")
    n, c, h, w = input.shape
    cout = weight.shape[0]
    offset = offset.contiguous()
    mask = mask.contiguous() if mask is not None else None
    grad_output = grad_output.contiguous()
    L = hip.lib()
    ws_bytes = L.otp_mdcn_backward_workspace_ex(n, c, h, w, cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                                                dilation_h, dilation_w, group, deformable_group, dtype, int(mask is not None))
    ws = torch.empty(max(int(ws_bytes), 8) // 8, dtype=torch.float64, device=input.device)
    st = L.otp_mdcn_backward_ex(
        hip.ptr(input), hip.ptr(offset), hip.ptr(mask), hip.ptr(weight), hip.ptr(grad_output),
        hip.ptr(grad_input), hip.ptr(grad_offset), hip.ptr(grad_mask), hip.ptr(grad_weight),
        hip.ptr(gb), hip.ptr(ws), ws_bytes,
        n, c, h, w, cout, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
        deformable_group, dtype, hip.stream_of(input))
    hip.check(st, "otp_mdcn_backward")


class ModulatedDeformConvFunction(Function):
    """autograd wrapper (reference thirdparty/deform_conv/functions/deform_conv.py:109-179)."""

    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1,
                groups=1, deformable_groups=1):
        ctx.stride, ctx.padding, ctx.dilation = stride, padding, dilation
        ctx.groups, ctx.deformable_groups = groups, deformable_groups
        ctx.with_bias = bias is not None
        if not input.is_cuda:
            raise NotImplementedError
        if not ctx.with_bias:
            bias = input.new_empty(1)
        if weight.requires_grad or mask.requires_grad or offset.requires_grad or input.requires_grad:
            ctx.save_for_backward(input, offset, mask, weight, bias)
        kh, kw = weight.shape[2:4]
        ho, wo = out_hw(input.shape[2], input.shape[3], kh, kw, stride, padding, dilation)
        output = input.new_empty((input.shape[0], weight.shape[0], ho, wo))
        modulated_deform_conv_cuda_forward(
            input.contiguous(), weight.contiguous(), bias, None, offset, mask, output, None, kh, kw,
            stride, stride, padding, padding, dilation, dilation, groups, deformable_groups, ctx.with_bias)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        input, offset, mask, weight, bias = ctx.saved_tensors
        grad_input = torch.empty_like(input)
        grad_offset = torch.empty_like(offset)
        grad_mask = torch.empty_like(mask)
        grad_weight = torch.zeros_like(weight)
        grad_bias = torch.zeros_like(bias)
        kh, kw = weight.shape[2:4]
        modulated_deform_conv_cuda_backward(
            input.contiguous(), weight.contiguous(), bias, None, offset, mask, None, grad_input,
            grad_weight, grad_bias, grad_offset, grad_mask, grad_output, kh, kw, ctx.stride, ctx.stride,
            ctx.padding, ctx.padding, ctx.dilation, ctx.dilation, ctx.groups, ctx.deformable_groups,
            ctx.with_bias)
        if not ctx.with_bias:
            grad_bias = None
        return grad_input, grad_offset, grad_mask, grad_weight, grad_bias, None, None, None, None, None


modulated_deform_conv = ModulatedDeformConvFunction.apply


# ---- DCN v1 (no modulation mask, no bias): the other three entry points of the reference's pybind module ----------
# The v1 kernels sample exactly like the modulated ones (same (-1, H) x (-1, W) window and corner tests:
# deform_conv_cuda_kernel.cu:22-51,166 vs :403-432,549), so they are the same HIP operator with mask == NULL: no mask
# stream is read and no mask gradient is written.
def deform_conv_forward_cuda(input, weight, offset, output, columns, ones, kW, kH, dW, dH, padW, padH, dilationW,
                             dilationH, group, deformable_group, im2col_step):
    """Reference pybind signature deform_conv_cuda.cpp:148-153 (returns 1).  ``columns`` / ``ones`` / ``im2col_step``
    are accepted and ignored: there is no im2col scratch and every image is one launch."""
    modulated_deform_conv_cuda_forward(input, weight, None, None, offset, None, output, None, kH, kW, dH, dW, padH, padW,
                                       dilationH, dilationW, group, deformable_group, False)
    return 1


def _v1_backward(input, offset, grad_output, weight, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group,
                 deformable_group):
    gi, go = torch.empty_like(input), torch.empty_like(offset)
    gw = torch.zeros_like(weight)
    modulated_deform_conv_cuda_backward(input, weight, None, None, offset, None, None, gi, gw, None, go, None, grad_output,
                                        kH, kW, dH, dW, padH, padW, dilationH, dilationW, group, deformable_group, False)
    return gi, go, gw


def deform_conv_backward_input_cuda(input, offset, gradOutput, gradInput, gradOffset, weight, columns, kW, kH, dW, dH,
                                    padW, padH, dilationW, dilationH, group, deformable_group, im2col_step):
    """Reference pybind signature deform_conv_cuda.cpp:251-257: overwrites gradInput / gradOffset (returns 1)."""
    gi, go, _ = _v1_backward(input, offset, gradOutput, weight, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group,
                             deformable_group)
    gradInput.copy_(gi)
    gradOffset.copy_(go)
    return 1


def deform_conv_backward_parameters_cuda(input, offset, gradOutput, gradWeight, columns, ones, kW, kH, dW, dH, padW, padH,
                                         dilationW, dilationH, group, deformable_group, scale, im2col_step):
    """Reference pybind signature deform_conv_cuda.cpp:364-370: gradWeight += scale * dL/dW (returns 1)."""
    # dL/dW does not depend on W; the input / offset gradients computed alongside are discarded
    _, _, gw = _v1_backward(input, offset, gradOutput, torch.zeros_like(gradWeight), kW, kH, dW, dH, padW, padH, dilationW,
                            dilationH, group, deformable_group)
    gradWeight.add_(gw, alpha=float(scale))
    return 1


class DeformConvFunction(Function):
    """autograd wrapper of DCN v1 (reference thirdparty/deform_conv/functions/deform_conv.py:10-107)."""

    @staticmethod
    def forward(ctx, input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, im2col_step=80):
        if input is not None and input.dim() != 4:
            raise ValueError("Expected 4D tensor as input, got {}D tensor instead.".format(input.dim()))
        if not input.is_cuda:
            raise NotImplementedError
        ctx.stride, ctx.padding, ctx.dilation = stride, padding, dilation
        ctx.groups, ctx.deformable_groups = groups, deformable_groups
        ctx.save_for_backward(input, offset, weight)
        kh, kw = weight.shape[2:4]
        ho, wo = out_hw(input.shape[2], input.shape[3], kh, kw, stride, padding, dilation)
        if ho <= 0 or wo <= 0:
            raise ValueError("convolution input is too small (output would be {}x{})".format(ho, wo))
        output = input.new_empty((input.shape[0], weight.shape[0], ho, wo))
        deform_conv_forward_cuda(input.contiguous(), weight.contiguous(), offset, output, None, None, kw, kh, stride, stride,
                                 padding, padding, dilation, dilation, groups, deformable_groups, im2col_step)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        input, offset, weight = ctx.saved_tensors
        kh, kw = weight.shape[2:4]
        gi, go, gw = _v1_backward(input.contiguous(), offset, grad_output, weight.contiguous(), kw, kh, ctx.stride, ctx.stride,
                                  ctx.padding, ctx.padding, ctx.dilation, ctx.dilation, ctx.groups, ctx.deformable_groups)
        return gi, go, gw, None, None, None, None, None, None


deform_conv = DeformConvFunction.apply


def dcn_fused_supported(cin, j, h, w, nd) -> bool:
    return bool(hip.lib().otp_dcn_fused_supported(int(cin), int(j), int(h), int(w), int(nd)))


def pack_dcn_fused(w_offs, w_masks, w_dcns, biases):
    """Per-dilation offset / mask conv weights ((18 J, 32, 3, 3) / (9 J, 32, 3, 3)), DCN weights (J, J, 3, 3) and biases (J or
    None) -> the packed image of :func:`dcn_fused` (csrc/dcn_fused.hip)."""
    nd, j = len(w_offs), w_dcns[0].shape[0]
    dev = w_offs[0].device
    require_gpu(*w_offs, *w_masks, *w_dcns)
    keep = [[_f32(t) for t in ts] for ts in (w_offs, w_masks, w_dcns, biases)]
    ptrs = [torch.tensor([0 if t is None else t.data_ptr() for t in ts], dtype=torch.int64, device=dev) for ts in keep]
    L = hip.lib()
    packed = _image(L.otp_dcn_fused_weight_bytes(nd, j), torch.int32, dev, RuntimeError, f"otp_dcn_fused: unsupported ND={nd}, J={j}")
    hip.check(L.otp_dcn_fused_pack(*[hip.ptr(t) for t in ptrs], hip.ptr(packed), nd, j, hip.stream_of(packed)),
              "otp_dcn_fused_pack")
    torch.cuda.current_stream(dev).synchronize()          # the pointer arrays and fp32 copies die with this frame
    return packed


def dcn_fused(trans, x, packed, dilations, alpha, out=None, workspace=None, stream=None):
    """out = alpha * sum over dilations of ModulatedDeformConv(x, Conv_off(trans), Conv_mask(trans)) + bias (SURVEY.md
    section 8 row f-2; model/OTPose.py:381-392) in one launch; the offsets and masks never reach HBM."""
    require_gpu(trans, x, packed)
    check_f32(trans)
    b, cin, h, w = trans.shape
    j = x.shape[1]
    L = hip.lib()
    out = torch.empty_like(x) if out is None else out
    nws = L.otp_dcn_fused_workspace(b, h, w)
    workspace = torch.empty(nws // 4, dtype=torch.int32, device=x.device) if workspace is None else workspace
    dl = (ctypes.c_int * len(dilations))(*[int(d) for d in dilations])
    hip.check(L.otp_dcn_fused_forward(hip.ptr(trans), hip.ptr(x), hip.ptr(packed), hip.ptr(out), hip.ptr(workspace), nws, b, cin, j,
                                      h, w, dl, len(dilations), float(alpha),
                                      stream if stream is not None else hip.stream_of(x)), "otp_dcn_fused_forward")
    return out
