"""Operator-level Python API over the C-ABI (mirror of the reference's native operator boundary).

``modulated_deform_conv`` replaces ``thirdparty.deform_conv.modulated_deform_conv``
(reference thirdparty/deform_conv/functions/deform_conv.py:109-179): same argument order, same
``NotImplementedError`` for CPU tensors (functions/deform_conv.py:131,149), same gradient tuple.
``modulated_deform_conv_cuda_forward`` / ``_backward`` keep the pybind entry points' names and
argument lists (reference thirdparty/deform_conv/src/deform_conv_cuda.cpp:474-480, 551-558) for
callers that bind the native module directly.
"""
from __future__ import annotations

import collections
import ctypes
import math
import os

import torch
from torch.autograd import Function

from . import hip
from .augment import FLIP_PAIRS

_K = hip.CONSTANTS              # the OTP_* integers of include/otpose_hip.h
_DTYPE_F32 = _K["OTP_DTYPE_F32"]


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NotImplementedError("otpose_amd operators run on the GPU only (no CPU path)")


def _check_f32(*tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"otpose_amd HIP operators are built for float32, got {t.dtype}")


def _out_hw(h, w, kh, kw, stride, pad, dil):
    """Output size of a convolution (the one statement of it: train_ops and bf16_ops call this too)."""
    return ((h + 2 * pad - (dil * (kh - 1) + 1)) // stride + 1,
            (w + 2 * pad - (dil * (kw - 1) + 1)) // stride + 1)


def _f32(t, device=None):
    """Detached contiguous fp32 form of an optional tensor, on ``device`` (default: where it is); ``None`` stays ``None``."""
    return None if t is None else t.detach().to(t.device if device is None else device, torch.float32).contiguous()


def _image(nbytes, dtype, device, exc, what, zero=False):
    """Storage of a packed image: ``nbytes`` is what the entry point's ``*_weight_bytes`` answered, 0 meaning that it has
    no kernel for the shape (``exc(what)``); 4-byte elements of ``dtype``, zero-filled on request."""
    if not nbytes:
        raise exc(what)
    return (torch.zeros if zero else torch.empty)(nbytes // 4, dtype=dtype, device=device)


_DTYPES = {torch.float32: _K["OTP_DTYPE_F32"], torch.float16: _K["OTP_DTYPE_F16"], torch.bfloat16: _K["OTP_DTYPE_BF16"],
           torch.float64: _K["OTP_DTYPE_F64"]}


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
    _require_gpu(input, weight, offset, mask, output)
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
    _require_gpu(input, weight, offset, mask, grad_output)
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
        ho, wo = _out_hw(input.shape[2], input.shape[3], kh, kw, stride, padding, dilation)
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
        ho, wo = _out_hw(input.shape[2], input.shape[3], kh, kw, stride, padding, dilation)
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


# ---- deformable PS-RoI pooling: the pybind entry points of the reference's second native module (deform_pool_cuda) ----------
_POOL_DTYPES = {torch.float32: _K["OTP_DTYPE_F32"], torch.float64: _K["OTP_DTYPE_F64"]}


def _pool_dtype(*tensors):
    """Storage type code of a pooling call: fp32 or fp64, one type for every tensor (the reference also dispatches half,
    deform_pool_cuda_kernel.cu:281; its half-precision coordinate arithmetic is not reproduced)."""
    ts = [t for t in tensors if t is not None]
    dt = ts[0].dtype
    if dt not in _POOL_DTYPES:
        raise RuntimeError(f"deformable RoI pooling is not implemented for {dt}")
    for t in ts:
        if t.dtype != dt:
            raise RuntimeError(f"deformable RoI pooling: mixed dtypes {dt} / {t.dtype}")
    return _POOL_DTYPES[dt]


def _pool_geometry(input, bbox, trans, out, no_trans, output_dim, group_size, pooled_size, part_size):
    """The shape checks of deform_pool_cuda.cpp:28-39 plus those its kernels leave to the caller; returns the C ABI's sizes."""
    if input.dim() != 4:
        raise RuntimeError(f"input tensor has to be 4-D, got {input.dim()}-D")
    if not input.is_contiguous():
        raise RuntimeError("input tensor has to be contiguous")
    n, c, h, w = input.shape
    num_bbox = bbox.shape[0]
    if bbox.dim() != 2 or bbox.shape[1] != 5:
        raise RuntimeError(f"bbox has to be (num_bbox, 5), got {tuple(bbox.shape)}")
    if num_bbox != out.shape[0]:
        raise RuntimeError(f"Output shape and bbox number wont match: ({out.shape[0]} vs {num_bbox}).")
    if tuple(out.shape[1:]) != (output_dim, pooled_size, pooled_size):
        raise RuntimeError(f"Output shape wont match: ({tuple(out.shape[1:])} vs {(output_dim, pooled_size, pooled_size)}).")
    if c != output_dim * group_size * group_size:
        raise RuntimeError(f"Input channels and output_dim * group_size^2 wont match: ({c} vs {output_dim * group_size ** 2}).")
    channels_trans = 2
    if not no_trans:
        if trans.dim() != 4 or trans.shape[0] != num_bbox or tuple(trans.shape[2:]) != (part_size, part_size):
            raise RuntimeError(f"Offset shape wont match: ({tuple(trans.shape)} vs ({num_bbox}, 2 * classes, {part_size}, "
                               f"{part_size})).")
        channels_trans = trans.shape[1]
        if channels_trans % 2 or channels_trans == 0 or output_dim % (channels_trans // 2):
            raise RuntimeError(f"Offset channels wont match: {channels_trans} channels for output_dim {output_dim}.")
    return n, c, h, w, num_bbox, channels_trans


def deform_psroi_pooling_cuda_forward(input, bbox, trans, out, top_count, no_trans, spatial_scale, output_dim, group_size,
                                      pooled_size, part_size, sample_per_part, trans_std):
    """In-place forward with the reference pybind signature (deform_pool_cuda.cpp:23-27): ``out`` and ``top_count`` are the
    caller's.  ``trans`` is ignored with ``no_trans`` (the reference's modules pass an empty tensor)."""
    no_trans = int(bool(no_trans))
    trans = None if no_trans else trans
    _require_gpu(input, bbox, trans, out, top_count)
    dtype = _pool_dtype(input, bbox, trans, out, top_count)
    n, c, h, w, num_bbox, channels_trans = _pool_geometry(input, bbox, trans, out, no_trans, output_dim, group_size,
                                                          pooled_size, part_size)
    if not (out.is_contiguous() and top_count.is_contiguous()):
        raise RuntimeError("output tensors have to be contiguous")
    if top_count.shape != out.shape:
        raise RuntimeError("top_count has to have the output's shape")
    if num_bbox == 0:
        return
    bbox = bbox.contiguous()
    trans = trans.contiguous() if trans is not None else None
    st = hip.lib().otp_deform_psroi_pool_forward(
        hip.ptr(input), hip.ptr(bbox), hip.ptr(trans), hip.ptr(out), hip.ptr(top_count), n, c, h, w, num_bbox, channels_trans,
        no_trans, float(spatial_scale), output_dim, group_size, pooled_size, part_size, sample_per_part, float(trans_std), dtype,
        hip.stream_of(input))
    hip.check(st, "otp_deform_psroi_pool_forward")


def deform_psroi_pooling_cuda_backward(out_grad, input, bbox, trans, top_count, input_grad, trans_grad, no_trans, spatial_scale,
                                       output_dim, group_size, pooled_size, part_size, sample_per_part, trans_std):
    """In-place backward with the reference pybind signature (deform_pool_cuda.cpp:47-52).  ``input_grad`` and ``trans_grad``
    are ADDED TO, as the reference's atomicAdd does (its Function passes zeros); ``trans_grad`` is untouched with
    ``no_trans``.  No float atomics: two calls on the same inputs return the same bits."""
    no_trans = int(bool(no_trans))
    trans = None if no_trans else trans
    trans_grad = None if no_trans else trans_grad
    _require_gpu(out_grad, input, bbox, trans, top_count, input_grad, trans_grad)
    dtype = _pool_dtype(out_grad, input, bbox, trans, top_count, input_grad, trans_grad)
    if not out_grad.is_contiguous():
        raise RuntimeError("out_grad tensor has to be contiguous")
    n, c, h, w, num_bbox, channels_trans = _pool_geometry(input, bbox, trans, out_grad, no_trans, output_dim, group_size,
                                                          pooled_size, part_size)
    if not input_grad.is_contiguous() or input_grad.shape != input.shape:
        raise RuntimeError("input_grad has to be contiguous and of the input's shape")
    if trans_grad is not None and (not trans_grad.is_contiguous() or trans_grad.shape != trans.shape):
        raise RuntimeError("trans_grad has to be contiguous and of the offset's shape")
    if top_count.shape != out_grad.shape:
        raise RuntimeError("top_count has to have the output's shape")
    if num_bbox == 0:
        return
    bbox = bbox.contiguous()
    trans = trans.contiguous() if trans is not None else None
    top_count = top_count.contiguous()
    L = hip.lib()
    geo = (n, c, h, w, num_bbox, channels_trans, no_trans)
    tail = (output_dim, group_size, pooled_size, part_size, sample_per_part)
    ws_bytes = L.otp_deform_psroi_pool_backward_workspace(*geo, *tail, dtype)
    ws = torch.empty(max(int(ws_bytes), 8) // 8, dtype=torch.float64, device=input.device)
    st = L.otp_deform_psroi_pool_backward(
        hip.ptr(out_grad), hip.ptr(input), hip.ptr(bbox), hip.ptr(trans), hip.ptr(top_count), hip.ptr(input_grad),
        hip.ptr(trans_grad), *geo, float(spatial_scale), *tail, float(trans_std), hip.ptr(ws), ws_bytes, dtype,
        hip.stream_of(input))
    hip.check(st, "otp_deform_psroi_pool_backward")


# ------------------------------------------------------------------------------------------------
# thin functional wrappers over the remaining C entry points (used by the engine and the tests)
# ------------------------------------------------------------------------------------------------
ACT_NONE, ACT_RELU, ACT_GELU = _K["OTP_ACT_NONE"], _K["OTP_ACT_RELU"], _K["OTP_ACT_GELU"]


class View:
    """A channel slice [coff, coff + C) of a contiguous (N, ctot, H, W) float32 tensor."""

    __slots__ = ("t", "coff", "C")

    def __init__(self, t, coff=0, C=None):
        assert t.is_contiguous() and t.dtype == torch.float32 and t.dim() == 4
        self.t, self.coff, self.C = t, coff, (t.shape[1] - coff if C is None else C)
        assert 0 <= coff and coff + self.C <= t.shape[1]

    @property
    def ctot(self):
        return self.t.shape[1]


# ---- launch arguments ------------------------------------------------------------------------------------------------------
# One ``*_args`` function per C entry point states its positional arguments (without the trailing stream) once: the eager
# wrappers below launch ``fn(*args, stream)`` at once, the inference engine records the same tuple for its launch list.
def _vp(v):
    """Device pointer of the tensor behind a :class:`View` / :class:`H8` (``None`` -> NULL)."""
    return None if v is None else hip.ptr(v.t)


def _slice(v):
    """(total channels, channel offset) of an optional :class:`View` / (groups, group offset) of an :class:`H8`."""
    return (0, 0) if v is None else (v.gtot, v.goff) if isinstance(v, H8) else (v.ctot, v.coff)


def _launch(fn, name, args, t, stream=None):
    """Launch now, on ``stream`` or on the stream PyTorch is enqueuing on for tensor ``t``'s device."""
    hip.check(fn(*args, stream if stream is not None else hip.stream_of(t)), name)


def pack_conv_weight(weight):
    """(Cout, Cin, kh, kw) -> packed [kh*kw][Cin][Cout16] device tensor for :func:`conv2d`."""
    _require_gpu(weight)
    _check_f32(weight)
    w = _f32(weight)
    if w.dim() == 3:                      # Conv1d weight (Cout, Cin, k) with k == 1
        w = w.unsqueeze(-1)
    cout, cin, kh, kw = w.shape
    cout16 = (cout + 15) // 16 * 16
    wp = torch.empty(kh * kw * cin * cout16, dtype=torch.float32, device=w.device)
    hip.check(hip.lib().otp_conv2d_pack_weight(hip.ptr(w), hip.ptr(wp), cout, cin, kh, kw, hip.stream_of(w)),
              "otp_conv2d_pack_weight")
    return wp


def conv_desc(inp: View, out: View, cout, kh, kw, stride, pad, dil, act=ACT_NONE, in2: View = None,
              res: View = None, res_up=1, frame_split=0, cin=None):
    d = hip.ConvDesc()
    n_in, _, h, w = inp.t.shape
    d.N = out.t.shape[0]
    d.Cin = inp.C if cin is None else cin
    d.H, d.W, d.Cout, d.kh, d.kw, d.stride, d.pad, d.dil = h, w, cout, kh, kw, stride, pad, dil
    d.in_ctot, d.in_coff = inp.ctot, inp.coff
    d.in2_ctot, d.in2_coff = (in2.ctot, in2.coff) if in2 is not None else (0, 0)
    d.out_ctot, d.out_coff = out.ctot, out.coff
    d.res_ctot, d.res_coff = (res.ctot, res.coff) if res is not None else (0, 0)
    d.res_up, d.act, d.frame_split = res_up, act, frame_split
    d.Ho, d.Wo = _out_hw(h, w, kh, kw, stride, pad, dil)
    f = max(res_up, 1)
    assert out.t.shape[2] == d.Ho * f and out.t.shape[3] == d.Wo * f, (tuple(out.t.shape), d.Ho, d.Wo, f)
    assert out.C == cout
    if res is not None:
        assert res.t.shape[2:] == out.t.shape[2:] and res.C == cout
    if in2 is not None:
        assert in2.t.shape[2:] == inp.t.shape[2:] and in2.C == d.Cin
    if frame_split:
        assert d.N == n_in * (inp.ctot // d.Cin)
    else:
        assert d.N == n_in
    return d


def conv2d_args(inp: View, wpacked, scale, shift, out: View, desc, in2: View = None, res: View = None):
    return (_vp(inp), _vp(in2), hip.ptr(wpacked), hip.ptr(scale), hip.ptr(shift), _vp(res), _vp(out), desc)


def conv2d_launch(inp: View, wpacked, scale, shift, out: View, desc, in2: View = None, res: View = None, stream=None):
    _launch(hip.lib().otp_conv2d, "otp_conv2d", conv2d_args(inp, wpacked, scale, shift, out, desc, in2, res), out.t, stream)


def pack_wino_weight(weight):
    """(Cout, Cin, 3, 3) -> U[16][Cin][Cout16] = G g G^T device tensor for :func:`conv2d_wino_launch`."""
    _require_gpu(weight)
    _check_f32(weight)
    w = _f32(weight)
    cout, cin, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    L = hip.lib()
    u = torch.empty(L.otp_conv2d_wino_weight_bytes(cout, cin) // 4, dtype=torch.float32, device=w.device)
    hip.check(L.otp_conv2d_wino_pack_weight(hip.ptr(w), hip.ptr(u), cout, cin, hip.stream_of(w)), "otp_conv2d_wino_pack_weight")
    return u


def small_conv_supported(desc) -> bool:
    return bool(hip.lib().otp_conv3x3_small_supported(desc))


def pack_small_conv_weight(weight):
    """(Cout, Cin, 3, 3) -> the [ci][tap][co] image :func:`conv3x3_small` reads through the scalar cache."""
    _require_gpu(weight)
    w = _f32(weight)
    cout, cin = w.shape[:2]
    L = hip.lib()
    wt = _image(L.otp_conv3x3_small_weight_bytes(cout, cin), torch.float32, w.device,
                ValueError, f"otp_conv3x3_small: unsupported channel counts ({cout}, {cin})")
    hip.check(L.otp_conv3x3_small_pack(hip.ptr(w), hip.ptr(wt), cout, cin, hip.stream_of(w)), "otp_conv3x3_small_pack")
    return wt


def conv3x3_small_args(inp: View, in2: View, wpacked, scale, shift, out: View, desc):
    return (_vp(inp), _vp(in2), hip.ptr(wpacked), hip.ptr(scale), hip.ptr(shift), _vp(out), desc)


def conv3x3_small(x, weight, scale=None, shift=None, act=ACT_NONE, in2=None):
    """act(scale * conv2d(x (+ in2), weight, 3x3, stride 1, pad 1) + shift) for <= 24 channels (csrc/conv_small.hip)."""
    _require_gpu(x, weight)
    _check_f32(x)
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    out = torch.empty(n, cout, h, w, dtype=torch.float32, device=x.device)
    iv, ov = View(x.contiguous()), View(out)
    i2 = View(in2.contiguous()) if in2 is not None else None
    d = conv_desc(iv, ov, cout, 3, 3, 1, 1, 1, act, i2)
    wt = pack_small_conv_weight(weight)
    _launch(hip.lib().otp_conv3x3_small, "otp_conv3x3_small", conv3x3_small_args(iv, i2, wt, scale, shift, ov, d), x)
    return out


def x3_weight_exponent(weight, scale=None) -> int:
    """The power of two k a layer's split-product weights are stored with: max |weight * scale| * 2^k lands in [2^13, 2^14).

    A weight is carried as two IEEE-half pieces hi + lo (csrc/common.h); `lo` is at most 2^-11 |w|, so for BatchNorm-folded
    weights of magnitude 1e-2 it is a SUBNORMAL half (spacing 2^-24) and the pair holds the weight to 2^-25 absolute - 17
    significand bits - and that error is the same for every pixel of every frame, so it does not average out over a layer's sum
    the way activation rounding does: it was the whole heat-map error of the split-product forward.  Scaled by
    2^k both pieces are normal (22 bits); the kernels multiply the accumulated sum by 2^-k (``otp_conv_desc.out_scale``; the
    pointwise kernels through their per-channel epilogue scale).  ``OTPOSE_X3_WSCALE=0`` stores the weights unscaled."""
    if os.environ.get("OTPOSE_X3_WSCALE", "1") == "0":
        return 0
    return h16_weight_exponent(weight, scale)


def _scaled_vec(scale, k, cout, device):
    """scale[cout] * 2^k as a contiguous fp32 vector (None when there is nothing to multiply by)"""
    sc = _f32(scale, device)
    if k == 0:
        return sc
    f = float(2.0 ** k)
    return sc * f if sc is not None else torch.full((cout,), f, dtype=torch.float32, device=device)


def pack_x3_weight(weight, scale=None, stride=1, k=0):
    """(Cout, Cin, k, k) fp32, k = 3 or 1 (times scale[cout] * 2^k) -> half hi / lo MFMA fragments for :func:`conv2d_x3_launch`
    (the chunking depends on the kernel size and the stride); the descriptor's ``out_scale`` must then be 2^-k
    (:func:`x3_weight_exponent`)."""
    _require_gpu(weight)
    _check_f32(weight)
    w = _f32(weight)
    if w.dim() == 3:
        w = w.unsqueeze(-1)
    cout, cin, kh, kw = w.shape
    assert kh == kw and kh in (1, 3)
    L = hip.lib()
    u = _image(L.otp_conv2d_x3_weight_bytes(cout, cin, kh, stride), torch.int32, w.device,
               ValueError, f"otp_conv2d_x3: unsupported channel counts ({cout}, {cin})")
    sc = _scaled_vec(scale, k, cout, w.device)
    hip.check(L.otp_conv2d_x3_pack_weight(hip.ptr(w), hip.ptr(sc), hip.ptr(u), cout, cin, kh, stride, hip.stream_of(w)),
              "otp_conv2d_x3_pack_weight")
    return u


def x3_supported(desc) -> bool:
    return bool(hip.lib().otp_conv2d_x3_supported(desc))


def conv2d_x3_args(inp: View, wpacked, shift, out: View, desc, res: View = None):
    return (_vp(inp), hip.ptr(wpacked), hip.ptr(shift), _vp(res), _vp(out), desc)


def conv2d_x3_launch(inp: View, wpacked, shift, out: View, desc, res: View = None, stream=None):
    _launch(hip.lib().otp_conv2d_x3, "otp_conv2d_x3", conv2d_x3_args(inp, wpacked, shift, out, desc, res), out.t, stream)


def conv2d_x3(x, weight, scale=None, shift=None, act=ACT_NONE, res=None, pad=1, dil=1, stride=1):
    """act(conv2d(x, weight, stride, pad, dil) * scale + shift + res) with split-half products (csrc/convx.hip)."""
    _require_gpu(x, weight)
    n, cin, h, w = x.shape
    cout, k = weight.shape[0], weight.shape[2]
    ho, wo = _out_hw(h, w, k, k, stride, pad, dil)
    out = torch.empty(n, cout, ho, wo, dtype=torch.float32, device=x.device)
    iv, ov = View(x.contiguous()), View(out)
    rv = View(res.contiguous()) if res is not None else None
    d = conv_desc(iv, ov, cout, k, k, stride, pad, dil, act, None, rv)
    e = x3_weight_exponent(weight, scale)
    d.out_scale = 2.0 ** -e
    conv2d_x3_launch(iv, pack_x3_weight(weight, scale, stride, e), shift, ov, d, rv)
    return out


# ---- split-record (S8) activations and the LDS-DMA fed 3x3 convolution (csrc/convs.hip) --------------------------------
S8_F32_C4, S8_F32_NCHW = _K["OTP_S8_F32_C4"], _K["OTP_S8_F32_NCHW"]


def s8_empty(n, c, h, w, device):
    """Storage of the S8 image of a logical (n, c, h, w) fp32 tensor: [n][c/8][2][h*w] records of 8 bf16 (hi | lo)."""
    nbytes = hip.lib().otp_s8_bytes(n, c, h, w)
    if not nbytes:
        raise ValueError(f"S8 images need a channel count that is a multiple of 8, got {c}")
    return torch.empty(nbytes // 4, dtype=torch.int32, device=device)


def c4_empty(n, c, h, w, device):
    """Storage of the C4 image [n][c/4][h*w][4] fp32 of a logical (n, c, h, w) tensor."""
    assert c % 4 == 0
    return torch.empty(n * c * h * w, dtype=torch.float32, device=device)


def s8_pack(inp, out=None, out_c4=None, stream=None):
    """fp32 NCHW tensor or channel-slice :class:`View` -> S8 image (hi = rne_bf16(x), lo = rne_bf16(x - hi)) and, when
    ``out_c4`` is given, the C4 image of the same values."""
    iv = inp if isinstance(inp, View) else View(inp.contiguous())
    _require_gpu(iv.t)
    n, _, h, w = iv.t.shape
    out = s8_empty(n, iv.C, h, w, iv.t.device) if out is None else out
    hip.check(hip.lib().otp_s8_pack(hip.ptr(iv.t), hip.ptr(out), hip.ptr(out_c4), n, iv.C, h, w, iv.ctot, iv.coff,
                                    stream if stream is not None else hip.stream_of(iv.t)), "otp_s8_pack")
    return out


def s8_unpack(s8, n, c, h, w):
    """S8 image -> fp32 (n, c, h, w) = hi + lo (tests / debugging)."""
    _require_gpu(s8)
    out = torch.empty(n, c, h, w, dtype=torch.float32, device=s8.device)
    hip.check(hip.lib().otp_s8_unpack(hip.ptr(s8), hip.ptr(out), n, c, h, w, hip.stream_of(s8)), "otp_s8_unpack")
    return out


def c4_unpack(c4, n, c, h, w):
    """C4 image -> fp32 NCHW (tests / debugging)."""
    _require_gpu(c4)
    out = torch.empty(n, c, h, w, dtype=torch.float32, device=c4.device)
    hip.check(hip.lib().otp_c4_unpack(hip.ptr(c4), hip.ptr(out), n, c, h, w, hip.stream_of(c4)), "otp_c4_unpack")
    return out


def s8_conv_supported(desc) -> bool:
    return bool(hip.lib().otp_conv3x3_s8_supported(desc))


def s8_conv_desc(n, cin, cout, h, w, act=ACT_NONE, out: View = None, res: View = None, stride=1):
    """Descriptor of the S8 convolutions: 3x3, pad 1, (n, cin, h, w) -> (n, cout, h / stride, w / stride)."""
    d = hip.ConvDesc()
    d.N, d.Cin, d.H, d.W, d.Cout = n, cin, h, w, cout
    d.kh = d.kw = 3
    d.stride, d.pad, d.dil = stride, 1, 1
    d.in_ctot, d.in_coff, d.in2_ctot, d.in2_coff = cin, 0, 0, 0
    d.out_ctot, d.out_coff = (out.ctot, out.coff) if out is not None else (cout, 0)
    d.res_ctot, d.res_coff = (res.ctot, res.coff) if res is not None else (0, 0)
    d.res_up = 1
    d.act, d.Ho, d.Wo, d.frame_split = act, h // stride, w // stride, 0
    return d


def s8_s2_conv_desc(n, cin, cout, h, w, act=ACT_NONE, out: View = None, res: View = None):
    """Descriptor of the stride-2 S8 convolution (csrc/convs2.hip): (n, cin, h, w) -> (n, cout, h / 2, w / 2)."""
    return s8_conv_desc(n, cin, cout, h, w, act, out, res, stride=2)


def s8_s2_conv_supported(desc, nchw_out=True):
    return bool(hip.lib().otp_conv3x3_s2_s8_supported(desc, int(nchw_out)))


def conv3x3_s2_s8_args(in_s8, wpacked, shift, desc, res: View = None, out: View = None, out_s8=None):
    """``out``: the fp32 NCHW result (with the optional residual ``res``), or ``out_s8``: its S8 image (csrc/convs2.hip)."""
    return (hip.ptr(in_s8), hip.ptr(wpacked), hip.ptr(shift), _vp(res), _vp(out), hip.ptr(out_s8), desc)


def conv3x3_s2_s8(x_s8, shape, weight, scale=None, shift=None, act=ACT_NONE, res=None, out="nchw"):
    """act(conv2d(x, weight, 3x3, stride 2, pad 1) * scale + shift (+ res)) from the S8 image ``x_s8`` of logical ``shape``
    (n, cin, h, w).  ``out = "nchw"``: fp32 (n, cout, h / 2, w / 2) tensor (``res`` an fp32 tensor of that shape or None);
    ``out = "s8"``: the S8 image of the result (no residual)."""
    _require_gpu(x_s8, weight)
    n, cin, h, w = shape
    cout = weight.shape[0]
    e = x3_weight_exponent(weight, scale)
    wp = pack_s8_weight(weight, scale, e)
    sh = shift.detach().contiguous().float() if shift is not None else None
    L = hip.lib()
    if out == "s8":
        assert res is None
        d = s8_s2_conv_desc(n, cin, cout, h, w, act)
        d.out_scale = 2.0 ** -e
        o8 = s8_empty(n, cout, h // 2, w // 2, x_s8.device)
        _launch(L.otp_conv3x3_s2_s8, "otp_conv3x3_s2_s8", conv3x3_s2_s8_args(x_s8, wp, sh, d, out_s8=o8), x_s8)
        return o8
    o = torch.empty(n, cout, h // 2, w // 2, dtype=torch.float32, device=x_s8.device)
    rv = View(res.contiguous()) if res is not None else None
    d = s8_s2_conv_desc(n, cin, cout, h, w, act, View(o), rv)
    d.out_scale = 2.0 ** -e
    _launch(L.otp_conv3x3_s2_s8, "otp_conv3x3_s2_s8", conv3x3_s2_s8_args(x_s8, wp, sh, d, rv, View(o)), x_s8)
    return o


def pack_s8_weight(weight, scale=None, k=0):
    """(Cout, Cin, 3, 3) fp32 (times scale[cout] * 2^k) -> half hi / lo MFMA fragments for :func:`conv3x3_s8_launch` and
    :func:`conv3x3_s2_s8`; the descriptor's ``out_scale`` must then be 2^-k (:func:`x3_weight_exponent`)."""
    _require_gpu(weight)
    _check_f32(weight)
    w = _f32(weight)
    cout, cin, kh, kw = w.shape
    assert kh == kw == 3
    L = hip.lib()
    u = _image(L.otp_conv3x3_s8_weight_bytes(cout, cin), torch.int32, w.device,
               ValueError, f"otp_conv3x3_s8: unsupported channel counts ({cout}, {cin})")
    sc = _scaled_vec(scale, k, cout, w.device)
    hip.check(L.otp_conv3x3_s8_pack_weight(hip.ptr(w), hip.ptr(sc), hip.ptr(u), cout, cin, hip.stream_of(w)),
              "otp_conv3x3_s8_pack_weight")
    return u


def conv3x3_s8_args(in_s8, wpacked, shift, desc, res=None, out_f32=None, f32_layout=S8_F32_C4, out_s8=None):
    """``res``: the residual's C4 image, or its S8 image with ``desc.res_layout = 1``; ``out_f32``: a C4 image or an NCHW tensor."""
    return (hip.ptr(in_s8), hip.ptr(wpacked), hip.ptr(shift), hip.ptr(res), hip.ptr(out_f32), f32_layout, hip.ptr(out_s8), desc)


def conv3x3_s8_launch(in_s8, wpacked, shift, desc, res_c4=None, out_f32=None, f32_layout=S8_F32_C4, out_s8=None, stream=None):
    _launch(hip.lib().otp_conv3x3_s8, "otp_conv3x3_s8",
            conv3x3_s8_args(in_s8, wpacked, shift, desc, res_c4, out_f32, f32_layout, out_s8), in_s8, stream)


def conv3x3_s8(x_s8, shape, weight, scale=None, shift=None, act=ACT_NONE, res_c4=None, f32="nchw", want_s8=True, res_s8=None):
    """act(conv2d(x, weight, 3x3, stride 1, pad 1) * scale + shift + res) from an S8 image ``x_s8`` of logical ``shape``
    (n, cin, h, w); ``res_c4`` a C4 image of the residual.  Returns (fp32 result - an NCHW tensor for f32 = "nchw", a C4 image
    for "c4", None for None -, S8 image of the result or None)."""
    _require_gpu(x_s8, weight)
    n, cin, h, w = shape
    cout = weight.shape[0]
    out = out_s8 = None
    layout = S8_F32_C4
    if f32 == "nchw":
        out, layout = torch.empty(n, cout, h, w, dtype=torch.float32, device=x_s8.device), S8_F32_NCHW
    elif f32 == "c4":
        out = c4_empty(n, cout, h, w, x_s8.device)
    if want_s8:
        out_s8 = s8_empty(n, cout, h, w, x_s8.device)
    d = s8_conv_desc(n, cin, cout, h, w, act)
    e = x3_weight_exponent(weight, scale)
    d.out_scale = 2.0 ** -e
    if res_s8 is not None:                           # the residual as S8 records (its hi + lo) instead of a C4 fp32 image
        assert res_c4 is None
        d.res_layout = 1
    conv3x3_s8_launch(x_s8, pack_s8_weight(weight, scale, e), shift, d, res_s8 if res_s8 is not None else res_c4, out, layout,
                      out_s8)
    return out, out_s8


def ln_mlp_args(y, gamma, beta, eps, packed, scale, shift, out, hid):
    """Arguments of otp_ln_mlp_fused / otp_ln_mlp_x3 / otp_ln_mlp_h1 on a (B, C, T) tensor."""
    b, c, t = y.shape
    return (hip.ptr(y), hip.ptr(gamma), hip.ptr(beta), eps, hip.ptr(packed), hip.ptr(scale), hip.ptr(shift), hip.ptr(out), b, c, hid, t)


def ln_mlp_fused(y, gamma, beta, eps, packed, scale, shift, out=None, hid=None, stream=None, entry="otp_ln_mlp_fused"):
    """out = y + scale * (W2 . gelu(W1 . LN(y) + b1)) + shift: ln2 + MLP + residual of TransformerBlock.forward
    (model/blocks.py:277-279) in one launch."""
    _require_gpu(y, packed)
    _check_f32(y)
    hid = 4 * y.shape[1] if hid is None else hid
    out = torch.empty_like(y) if out is None else out
    _launch(getattr(hip.lib(), entry), entry, ln_mlp_args(y, gamma, beta, eps, packed, scale, shift, out, hid), y, stream)
    return out


def dense_cc_supported(c, t) -> bool:
    return bool(hip.lib().otp_dense_cc_supported(int(c), int(t)))


def dense_x3_supported(c, t) -> bool:
    return bool(hip.lib().otp_dense_x3_supported(int(c), int(t)))


def pack_dense_cc(weight, scale=None, shift=None, x3=False, grad=False):
    """(C, C[, 1]) pointwise weight (+ per-output-channel scale / shift) -> the per-16-row fragment image of
    :func:`dense_cc` (MaskedMHCA query / key / value / proj, model/blocks.py:383-386).  ``x3``: the split-half image of
    csrc/densex.hip (pass the same flag to :func:`dense_cc` / :func:`qkv_front`); ``grad`` (with ``x3``): the image with
    bfloat16 pieces for :func:`dense_cc` on operands of unknown magnitude - gradients (otp_bf16_pieces in csrc/densex.hip)."""
    _require_gpu(weight)
    c = weight.shape[0]
    L = hip.lib()
    entry = ("otp_dense_x3_pack_bf16p" if grad else "otp_dense_x3_pack") if x3 else "otp_dense_cc_pack"
    nbytes = (L.otp_dense_x3_weight_bytes if x3 else L.otp_dense_cc_weight_bytes)(c) if weight.shape[1] == c else 0
    packed = _image(nbytes, torch.float32, weight.device, RuntimeError, f"otp_dense_cc: unsupported weight shape {tuple(weight.shape)}")
    w, sc, sh = (_f32(t, weight.device) for t in (weight, scale, shift))
    hip.check(getattr(L, entry)(hip.ptr(w), hip.ptr(sc), hip.ptr(sh), hip.ptr(packed), c, hip.stream_of(w)), entry)
    return packed


def dense_cc_args(xs, packs, ress, outs):
    """ctypes pointer arrays for :func:`dense_cc_launch` (kept by the caller while launches may still be issued)."""
    n = len(xs)
    arr = lambda ts: (ctypes.c_void_p * n)(*[hip.ptr(t) for t in ts])     # noqa: E731
    return arr(xs), arr(packs), arr(ress if ress is not None else [None] * n), arr(outs)


def dense_cc(xs, packs, ress=None, outs=None, stream=None, x3=False, grad=False, half=False):
    """out[p] = scale[p] * (W[p] . x[p]) + shift[p] (+ res[p]) for up to three (B, C, T) problems in one launch (``grad``: see
    :func:`pack_dense_cc`; ``half`` with ``x3``: the fp16 engine's arithmetic - operands rounded to half once, otp_dense_h1)."""
    _require_gpu(*xs)
    b, c, t = xs[0].shape
    outs = [torch.empty_like(x) for x in xs] if outs is None else outs
    ax, ap, ar, ao = dense_cc_args(xs, packs, ress, outs)
    entry = ("otp_dense_x3_bf16p" if grad else "otp_dense_h1" if half else "otp_dense_x3") if x3 else "otp_dense_cc"
    hip.check(getattr(hip.lib(), entry)(ax, ap, ar, ao, len(xs), b, c, t, stream if stream is not None else hip.stream_of(xs[0])), entry)
    return outs


def stem_conv_x3_supported(b, f, h, w, cout) -> bool:
    return bool(hip.lib().otp_stem_conv_x3_supported(int(b), int(f), int(h), int(w), int(cout)))


def pack_stem_conv_x3(weight, scale=None, shift=None):
    """(Cout, 3, 3, 3) weight of HRNet's first conv (+ folded BatchNorm) -> the register image of :func:`stem_conv_x3`."""
    _require_gpu(weight)
    cout = weight.shape[0]
    L = hip.lib()
    nbytes = L.otp_stem_conv_x3_weight_bytes(cout) if tuple(weight.shape[1:]) == (3, 3, 3) else 0
    packed = _image(nbytes, torch.float32, weight.device, RuntimeError, f"otp_stem_conv_x3: unsupported weight shape {tuple(weight.shape)}")
    w, sc, sh = (_f32(t, weight.device) for t in (weight, scale, shift))
    hip.check(L.otp_stem_conv_x3_pack(hip.ptr(w), hip.ptr(sc), hip.ptr(sh), hip.ptr(packed), cout, hip.stream_of(w)),
              "otp_stem_conv_x3_pack")
    return packed


def stem_conv_x3_args(clip, packed, out, frames, cout):
    """Arguments of otp_stem_conv_x3 / otp_h16_stem: ``clip`` (B, 3 * frames, H, W) fp32, ``out`` a tensor or an :class:`H8`."""
    b, _, h, w = clip.shape
    return (hip.ptr(clip), hip.ptr(packed), hip.ptr(out.t if isinstance(out, H8) else out), b, frames, h, w, cout)


def stem_conv_x3(clip, packed, cout, frames=5, out=None, stream=None):
    """relu(bn(conv3x3 stride 2 pad 1)) of the 3-channel frames of ``clip`` (B, 3 * frames, H, W) -> (frames * B, cout, Ho, Wo),
    frame-major like model/OTPose.py:317."""
    _require_gpu(clip)
    b, c, h, w = clip.shape
    assert c == 3 * frames and clip.is_contiguous() and clip.dtype == torch.float32
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = torch.empty(frames * b, cout, ho, wo, dtype=torch.float32, device=clip.device) if out is None else out
    _launch(hip.lib().otp_stem_conv_x3, "otp_stem_conv_x3", stem_conv_x3_args(clip, packed, out, frames, cout), clip, stream)
    return out


def pointwise_x3_supported(cin, cout, t) -> bool:
    return bool(hip.lib().otp_pointwise_x3_supported(int(cin), int(cout), int(t)))


def _pointwise_operands(weight, scale, shift, cout, cin, device):
    """fp32 (cout, cin) weight, scale, shift of a pointwise packer on ``device``: the weights stored times 2^e
    (:func:`x3_weight_exponent`), undone by the kernel's per-channel epilogue scale."""
    w, sc, sh = _f32(weight, device).reshape(cout, cin), _f32(scale, device), _f32(shift, device)
    e = x3_weight_exponent(w)
    if e:
        w, sc = w * float(2.0 ** e), _scaled_vec(sc, -e, cout, w.device)
    return w, sc, sh


def _pack_pointwise(entry, weight, scale, shift):
    """(Cout, Cin[, 1, 1]) weight (+ per-output-channel scale / shift) -> the image ``<entry>_pack`` writes."""
    _require_gpu(weight)
    cout, cin = weight.shape[:2]
    L = hip.lib()
    packed = _image(getattr(L, entry + "_weight_bytes")(cin, cout), torch.float32, weight.device,
                    RuntimeError, f"{entry}: unsupported weight shape {tuple(weight.shape)}")
    w, sc, sh = _pointwise_operands(weight, scale, shift, cout, cin, weight.device)
    hip.check(getattr(L, entry + "_pack")(hip.ptr(w), hip.ptr(sc), hip.ptr(sh), hip.ptr(packed), cin, cout, hip.stream_of(w)),
              entry + "_pack")
    return packed


def pack_pointwise_x3(weight, scale=None, shift=None):
    """(Cout, Cin[, 1, 1]) weight (+ per-output-channel scale / shift, e.g. a folded BatchNorm) -> the block image of
    :func:`pointwise_x3` (HRNet layer1's 1x1 convs, model/HRNet.py:551-571)."""
    return _pack_pointwise("otp_pointwise_x3", weight, scale, shift)


def pointwise_x3_args(x: View, packed, out: View, res: View = None, relu=False):
    b, _, h, w = x.t.shape
    return (_vp(x), hip.ptr(packed), _vp(res), _vp(out), b, x.C, out.C, h * w, x.ctot, x.coff, *_slice(res), out.ctot, out.coff,
            int(bool(relu)))


def pointwise_x3(x: View, packed, out: View, res: View = None, relu=False, stream=None):
    """out = act(scale * (W . x) + shift (+ res)) over channel-slice views of (B, ctot, H, W) fp32 tensors."""
    _require_gpu(x.t, out.t)
    _launch(hip.lib().otp_pointwise_x3, "otp_pointwise_x3", pointwise_x3_args(x, packed, out, res, relu), x.t, stream)
    return out


def pointwise_x3_s8_supported(cin, cout, t) -> bool:
    return bool(hip.lib().otp_pointwise_x3_s8_supported(int(cin), int(cout), int(t)))


def pack_pointwise_x3_s8(weight, scale=None, shift=None):
    """Weight image of :func:`pointwise_x3_s8` (its own row order: pairs of 16-row tiles interleaved by groups of 4)."""
    return _pack_pointwise("otp_pointwise_x3_s8", weight, scale, shift)


def pointwise_x3_s8_res_args(x: View, packed, cout, out_s8, res: View = None, relu=False):
    b, _, h, w = x.t.shape
    return (_vp(x), hip.ptr(packed), _vp(res), hip.ptr(out_s8), b, x.C, cout, h * w, x.ctot, x.coff, *_slice(res), int(bool(relu)))


def pointwise_x3_s8(x: View, packed, cout, out_s8=None, relu=False, stream=None, res: View = None):
    """S8 image of act(scale * (W . x) + shift (+ res)): a 1x1 conv feeding :func:`conv3x3_s8_launch` without an fp32 round trip
    (``res``: an fp32 NCHW channel-slice view, a Bottleneck's conv3)."""
    _require_gpu(x.t)
    b, _, h, w = x.t.shape
    out_s8 = s8_empty(b, cout, h, w, x.t.device) if out_s8 is None else out_s8
    _launch(hip.lib().otp_pointwise_x3_s8_res, "otp_pointwise_x3_s8_res", pointwise_x3_s8_res_args(x, packed, cout, out_s8, res, relu),
            x.t, stream)
    return out_s8


def pointwise_x3_pair_supported(cin, cmid, cout2, t) -> bool:
    return bool(hip.lib().otp_pointwise_x3_pair_supported(int(cin), int(cmid), int(cout2), int(t)))


def pack_pointwise_x3_pair(weight1, scale1, shift1, weight2, scale2=None, shift2=None):
    """Weight image of :func:`pointwise_x3_pair`: conv3 (Cmid, Cin) of one Bottleneck and conv1 (Cout2, Cmid) of the next, each
    with its folded BatchNorm - the two images of :func:`pack_pointwise_x3_s8` in one buffer."""
    _require_gpu(weight1, weight2)
    cmid, cin = weight1.shape[:2]
    cout2 = weight2.shape[0]
    L = hip.lib()
    nbytes = L.otp_pointwise_x3_pair_weight_bytes(cin, cmid, cout2) if weight2.shape[1] == cmid else 0
    packed = _image(nbytes, torch.float32, weight1.device, RuntimeError,
                    f"otp_pointwise_x3_pair: unsupported weight shapes {tuple(weight1.shape)}, {tuple(weight2.shape)}")
    ws = [*_pointwise_operands(weight1, scale1, shift1, cmid, cin, weight1.device),
          *_pointwise_operands(weight2, scale2, shift2, cout2, cmid, weight1.device)]
    hip.check(L.otp_pointwise_x3_pair_pack(*[hip.ptr(t) for t in ws], hip.ptr(packed), cin, cmid, cout2, hip.stream_of(ws[0])),
              "otp_pointwise_x3_pair_pack")
    return packed


def pointwise_x3_pair_args(x: View, packed, out: View, cout2, out_s8, res: View = None, relu1=True, relu2=True):
    b, _, h, w = x.t.shape
    return (_vp(x), hip.ptr(packed), _vp(res), _vp(out), hip.ptr(out_s8), b, x.C, out.C, cout2, h * w, x.ctot, x.coff, *_slice(res),
            out.ctot, out.coff, int(bool(relu1)), int(bool(relu2)))


def pointwise_x3_pair(x: View, packed, out: View, cout2, res: View = None, out_s8=None, relu1=True, relu2=True, stream=None):
    """out = act1(scale1 * (W1 . x) + shift1 (+ res)) as :func:`pointwise_x3` writes it AND the S8 image of
    act2(scale2 * (W2 . out) + shift2) as :func:`pointwise_x3_s8` of ``out`` writes it, in one launch; returns the S8 image."""
    _require_gpu(x.t, out.t)
    b, _, h, w = x.t.shape
    out_s8 = s8_empty(b, cout2, h, w, x.t.device) if out_s8 is None else out_s8
    _launch(hip.lib().otp_pointwise_x3_pair, "otp_pointwise_x3_pair",
            pointwise_x3_pair_args(x, packed, out, cout2, out_s8, res, relu1, relu2), x.t, stream)
    return out_s8


def pack_qkv_table(dwq, dwk, dwv, gq, bq, gk, bk, gv, bv):
    """Depthwise (C, 1, 3) weights and LayerNorm (C) gamma / beta of MaskedMHCA's query / key / value paths
    (model/blocks.py:359-381) -> the per-channel table of :func:`qkv_front`."""
    ts = [_f32(t) for t in (dwq, dwk, dwv, gq, bq, gk, bk, gv, bv)]
    _require_gpu(*ts)
    c = ts[3].numel()
    L = hip.lib()
    table = torch.empty(L.otp_qkv_front_table_bytes(c) // 4, dtype=torch.float32, device=ts[0].device)
    hip.check(L.otp_qkv_front_pack_table(*[hip.ptr(t) for t in ts], hip.ptr(table), c, hip.stream_of(ts[0])),
              "otp_qkv_front_pack_table")
    return table


def qkv_front_args(x, table, packs, outs, eps):
    """Arguments of otp_qkv_front / otp_qkv_front_x3 / otp_qkv_front_h1."""
    b, c, t = x.shape
    return (hip.ptr(x), hip.ptr(table), *[hip.ptr(p) for p in packs], *[hip.ptr(o) for o in outs], b, c, t, eps)


def qkv_front(x, table, packs, eps=1e-5, outs=None, stream=None, x3=False, half=False):
    """q, k, v = W_p . LN_p(dwconv3_p(x)) + b_p (stride 1) in one launch; ``packs`` = three :func:`pack_dense_cc` images
    (``half`` with ``x3``: operands rounded to half once, otp_qkv_front_h1)."""
    _require_gpu(x, table)
    outs = [torch.empty_like(x) for _ in range(3)] if outs is None else outs
    entry = ("otp_qkv_front_h1" if half else "otp_qkv_front_x3") if x3 else "otp_qkv_front"
    _launch(getattr(hip.lib(), entry), entry, qkv_front_args(x, table, packs, outs, eps), x, stream)
    return outs


def mlp_fused_supported(c, hid, t) -> bool:
    return bool(hip.lib().otp_mlp_fused_supported(int(c), int(hid), int(t)))


def pack_mlp_weights(w1, b1, w2):
    """Conv1d(C,4C,1) / Conv1d(4C,C,1) weights of a TransformerBlock MLP (model/blocks.py:248-254) -> the per-hidden-block
    fragment image :func:`mlp_fused` streams through LDS."""
    _require_gpu(w1, b1, w2)
    hid, c = w1.shape[:2]
    L = hip.lib()
    packed = _image(L.otp_mlp_fused_weight_bytes(c, hid), torch.float32, w1.device,
                    RuntimeError, f"otp_mlp_fused: unsupported widths C={c}, HID={hid}")
    w1c, w2c, b1c = (_f32(t) for t in (w1, w2, b1))
    hip.check(L.otp_mlp_fused_pack(hip.ptr(w1c), hip.ptr(b1c), hip.ptr(w2c), hip.ptr(packed), c, hid, hip.stream_of(w1c)),
              "otp_mlp_fused_pack")
    return packed


def mlp_fused(x, packed, scale, shift, res, out=None, hid=None, stream=None, entry="otp_mlp_fused"):
    """out = res + scale * (W2 . gelu(W1 . x + b1)) + shift on (B, C, T) tensors, one launch (eval-mode MLP half of
    TransformerBlock.forward, model/blocks.py:277-279)."""
    _require_gpu(x, packed, res)
    _check_f32(x)
    b, c, t = x.shape
    hid = 4 * c if hid is None else hid
    out = torch.empty_like(x) if out is None else out
    _launch(getattr(hip.lib(), entry), entry, (hip.ptr(x), hip.ptr(packed), hip.ptr(scale), hip.ptr(shift), hip.ptr(res), hip.ptr(out),
                                                b, c, hid, t), x, stream)
    return out


def dcn_fused_supported(cin, j, h, w, nd) -> bool:
    return bool(hip.lib().otp_dcn_fused_supported(int(cin), int(j), int(h), int(w), int(nd)))


def pack_dcn_fused(w_offs, w_masks, w_dcns, biases):
    """Per-dilation offset / mask conv weights ((18 J, 32, 3, 3) / (9 J, 32, 3, 3)), DCN weights (J, J, 3, 3) and biases (J or
    None) -> the packed image of :func:`dcn_fused` (csrc/dcn_fused.hip)."""
    nd, j = len(w_offs), w_dcns[0].shape[0]
    dev = w_offs[0].device
    _require_gpu(*w_offs, *w_masks, *w_dcns)
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
    _require_gpu(trans, x, packed)
    _check_f32(trans)
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


def mlp_x3_supported(c, hid, t) -> bool:
    return bool(hip.lib().otp_mlp_x3_supported(int(c), int(hid), int(t)))


def pack_mlp_x3_weights(w1, b1, w2, half=False):
    """The same MLP weights as :func:`pack_mlp_weights`, split into half hi / lo MFMA fragments per 32 hidden channels
    (csrc/mlpx.hip); ``half``: the hi-only image of the fp16 engine's form (``ln_mlp_x3(..., half=True)``)."""
    _require_gpu(w1, b1, w2)
    hid, c = w1.shape[:2]
    L = hip.lib()
    entry = "otp_mlp_h1" if half else "otp_mlp_x3"
    packed = _image(getattr(L, entry + "_weight_bytes")(c, hid), torch.int32, w1.device,
                    RuntimeError, f"otp_mlp_x3: unsupported widths C={c}, HID={hid}")
    w1c, w2c, b1c = (_f32(t) for t in (w1, w2, b1))
    hip.check(getattr(L, entry + "_pack")(hip.ptr(w1c), hip.ptr(b1c), hip.ptr(w2c), hip.ptr(packed), c, hid, hip.stream_of(w1c)),
              entry + "_pack")
    return packed


def mlp_x3(x, packed, scale, shift, res, out=None, hid=None, stream=None):
    """:func:`mlp_fused` with split-half products on the 16-bit matrix cores (fp32 storage / accumulation)."""
    return mlp_fused(x, packed, scale, shift, res, out, hid, stream, "otp_mlp_x3")


def ln_mlp_x3(y, gamma, beta, eps, packed, scale, shift, out=None, hid=None, stream=None, half=False):
    """:func:`ln_mlp_fused` with split-half products (``half``: operands and the hidden layer rounded to half once, otp_ln_mlp_h1)."""
    return ln_mlp_fused(y, gamma, beta, eps, packed, scale, shift, out, hid, stream, "otp_ln_mlp_h1" if half else "otp_ln_mlp_x3")


def wino_supported(desc) -> bool:
    return bool(hip.lib().otp_conv2d_wino_supported(desc))


def winograd_pays(cin, cout):
    """Shapes on which the Winograd kernel measured faster than the direct one (tools/conv_bench.py --wino): whole
    8-channel chunks and output-channel counts that fill its 48-row tiles (64 -> 64 would compute 96 rows)."""
    cout16 = (cout + 15) // 16 * 16
    if cin == 64 and cout16 == 64:
        return True                                   # layer1 Bottleneck conv2: 0.463 -> 0.408 ms despite the ragged 2nd tile
    return cin >= 32 and cin % 8 == 0 and cout16 >= 48 and ((cout16 + 47) // 48) * 48 <= 1.15 * cout16


def runs_winograd(enabled, cin, cout, desc) -> bool:
    """The one rule for "this convolution runs on the Winograd kernel" (inference engine and training operators alike): the
    OTPOSE_WINOGRAD switch is on (``enabled``), 3x3 / stride 1 / pad 1 / dilation 1, the shape pays and the kernel takes it."""
    return bool(enabled and (desc.kh, desc.kw, desc.stride, desc.pad, desc.dil) == (3, 3, 1, 1, 1)
                and winograd_pays(cin, cout) and wino_supported(desc))


def conv2d_wino_args(inp: View, upacked, scale, shift, out: View, desc, res: View = None):
    return (_vp(inp), hip.ptr(upacked), hip.ptr(scale), hip.ptr(shift), _vp(res), _vp(out), desc)


def conv2d_wino_launch(inp: View, upacked, scale, shift, out: View, desc, res: View = None, stream=None):
    _launch(hip.lib().otp_conv2d_wino, "otp_conv2d_wino", conv2d_wino_args(inp, upacked, scale, shift, out, desc, res), out.t, stream)


def conv2d_wino(x, weight, scale=None, shift=None, act=ACT_NONE, res=None):
    """3x3 / stride 1 / pad 1 convolution through the Winograd F(2x2, 3x3) kernel, fresh output."""
    _require_gpu(x, weight)
    cout = weight.shape[0]
    out = torch.empty((x.shape[0], cout, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
    iv, ov = View(x.contiguous()), View(out)
    rv = View(res.contiguous()) if res is not None else None
    d = conv_desc(iv, ov, cout, 3, 3, 1, 1, 1, act, None, rv, 1)
    conv2d_wino_launch(iv, pack_wino_weight(weight), scale, shift, ov, d, rv)
    return out


def conv2d(x, weight, scale=None, shift=None, stride=1, pad=0, dil=1, act=ACT_NONE, res=None, in2=None, res_up=1):
    """Convenience form: out = act(scale * conv(x (+ in2), weight) + shift (+ res)), fresh output."""
    _require_gpu(x, weight)
    w4 = weight if weight.dim() == 4 else weight.unsqueeze(-1)
    cout, cin, kh, kw = w4.shape
    h, w = x.shape[2:]
    ho, wo = _out_hw(h, w, kh, kw, stride, pad, dil)
    out = torch.empty((x.shape[0], cout, ho * max(res_up, 1), wo * max(res_up, 1)), dtype=torch.float32, device=x.device)
    iv, ov = View(x.contiguous()), View(out)
    rv = View(res.contiguous()) if res is not None else None
    i2 = View(in2.contiguous()) if in2 is not None else None
    d = conv_desc(iv, ov, cout, kh, kw, stride, pad, dil, act, i2, rv, res_up)
    conv2d_launch(iv, pack_conv_weight(w4), scale, shift, ov, d, i2, rv)
    return out


def upsample_add_args(low: View, res: View, out: View, f, relu=False):
    n, _, hl, wl = low.t.shape
    return (_vp(low), _vp(res), _vp(out), n, low.C, hl, wl, f, int(relu), low.ctot, low.coff, res.ctot, res.coff, out.ctot, out.coff)


def upsample_add(low, res, f, relu=False, out=None):
    """out = act(res + nearest_upsample_f(low)) (HRNet fuse accumulate for f >= 4); ``out`` may be ``res``."""
    _require_gpu(low, res)
    out = torch.empty_like(res) if out is None else out
    _launch(hip.lib().otp_upsample_add, "otp_upsample_add", upsample_add_args(View(low), View(res), View(out), f, relu), low)
    return out


def upsample_add_multi_args(lows, factors, res: View, out: View, relu=False):
    """(arguments, ctypes arrays the caller keeps alive while the launch may still be issued); ``lows``: whole-tensor Views."""
    n, _, hh, wh = out.t.shape
    lp = (ctypes.c_void_p * len(lows))(*[_vp(v) for v in lows])
    fp = (ctypes.c_int * len(lows))(*[int(f) for f in factors])
    return (lp, fp, len(lows), _vp(res), _vp(out), n, res.C, hh, wh, int(relu), res.ctot, res.coff, out.ctot, out.coff), (lp, fp)


def upsample_add_multi(lows, res, relu=False, out=None):
    """out = act(res + sum_k nearest_upsample(lows[k])) in one pass (an HRNet fuse row's upsampled terms, summed in list
    order); each ``lows[k]`` is (N, C, H / f_k, W / f_k) with f_k a power of two >= 2."""
    _require_gpu(res, *lows)
    n, c, hh, wh = res.shape
    out = torch.empty_like(res) if out is None else out
    lows = [t.contiguous() for t in lows]
    args, _keep = upsample_add_multi_args([View(t) for t in lows], [hh // t.shape[2] for t in lows], View(res), View(out), relu)
    _launch(hip.lib().otp_upsample_add_multi, "otp_upsample_add_multi", args, res)
    return out


def ln_channel(x, gamma, beta, eps=1e-5, pool=False):
    _require_gpu(x)
    b, c, t = x.shape
    y = torch.empty_like(x)
    p = torch.empty((b, c, (t + 2 - 3) // 2 + 1), dtype=x.dtype, device=x.device) if pool else None
    hip.check(hip.lib().otp_ln_channel(hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), hip.ptr(y), hip.ptr(p), b, c, t,
                                       eps, hip.stream_of(x)), "otp_ln_channel")
    return (y, p) if pool else y


def dwconv_ln3(x, dw, gammas, betas, stride, eps=1e-5):
    """dw / gammas / betas: triples for (query, key, value)."""
    _require_gpu(x)
    b, c, t = x.shape
    to = (t + 2 - 3) // stride + 1
    outs = [torch.empty((b, c, to), dtype=x.dtype, device=x.device) for _ in range(3)]
    hip.check(hip.lib().otp_dwconv_ln3(
        hip.ptr(x), hip.ptr(dw[0]), hip.ptr(dw[1]), hip.ptr(dw[2]), hip.ptr(gammas[0]), hip.ptr(betas[0]),
        hip.ptr(gammas[1]), hip.ptr(betas[1]), hip.ptr(gammas[2]), hip.ptr(betas[2]), hip.ptr(outs[0]),
        hip.ptr(outs[1]), hip.ptr(outs[2]), b, c, t, stride, eps, hip.stream_of(x)), "otp_dwconv_ln3")
    return outs


def chan_attn_args(q, k, v, out, ws, nbytes, n_head, scale):
    b, c, t = q.shape
    return (hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(out), hip.ptr(ws), nbytes, b, c, t, n_head, scale)


def chan_attn(q, k, v, n_head, scale):
    _require_gpu(q, k, v)
    b, c, t = q.shape
    out = torch.empty_like(q)
    L = hip.lib()
    nbytes = L.otp_chan_attn_workspace(b, c, t, n_head)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=q.device)
    _launch(L.otp_chan_attn, "otp_chan_attn", chan_attn_args(q, k, v, out, ws, nbytes, n_head, scale), q)
    return out


def check_local_attn(c, t, n_head, window_size):
    """Raise ``ValueError`` for a shape the local attention does not take (odd window 5 .. 33, ``t % (window_size - 1) == 0``:
    ``otp_local_attn_supported``)."""
    if n_head <= 0 or c % n_head:
        raise ValueError(f"local_attn: {c} channels do not split into {n_head} heads")
    if not hip.lib().otp_local_attn_supported(c // n_head, t, int(window_size)):
        raise ValueError(f"local_attn: window_size must be odd and in [5, 33] and the {t} tokens a multiple of window_size - 1, "
                         f"got window_size {window_size}")


def local_attn_args(q, k, v, rel_pe, out, probs, n_head, window_size, scale):
    b, c, t = q.shape
    return (hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(rel_pe), hip.ptr(out), hip.ptr(probs), b, c, t, n_head, int(window_size),
            scale)


def _rel_pe_table(rel_pe, n_head, window_size, like):
    """``rel_pe`` ((1, 1, n_head, window_size) parameter or None) as the contiguous fp32 (n_head, window_size) table."""
    if rel_pe is None:
        return None
    if rel_pe.numel() != n_head * window_size:
        raise ValueError(f"local_attn: rel_pe has {rel_pe.numel()} entries, n_head * window_size is {n_head * window_size}")
    return rel_pe.detach().to(like.device, torch.float32).reshape(n_head, window_size).contiguous()


def local_attn(q, k, v, n_head, window_size, scale, rel_pe=None):
    """Local-window attention of LocalMaskedMHCA (model/blocks.py:479-833) on q, k, v (B, C, T): every token attends to the
    ``window_size`` positions centred on it, positions outside the sequence take no part; ``rel_pe`` (1, 1, n_head, window_size)
    is added to the scaled scores.  Returns (B, C, T) in the natural layout (csrc/localattn.hip, one launch)."""
    _require_gpu(q, k, v)
    _check_f32(q, k, v)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    b, c, t = q.shape
    check_local_attn(c, t, n_head, window_size)
    rel = _rel_pe_table(rel_pe, n_head, window_size, q)
    out = torch.empty_like(q)
    _launch(hip.lib().otp_local_attn, "otp_local_attn", local_attn_args(q, k, v, rel, out, None, n_head, window_size, scale), q)
    return out


CONV_EMBD_KS = (1, 3, 5)              # the kernel sizes csrc/convembd.hip is built for
CONV_EMBD_MAX_CHANNELS = 256


def check_conv_embd(b, cin, h, w, cout, ks):
    """Raise ``ValueError`` for a shape the conv embedding does not take (``otp_conv_embd_supported``: ks 1 / 3 / 5, at most 256
    input and output channels)."""
    if (isinstance(ks, bool) or not isinstance(ks, int) or min(b, cin, h, w, cout) < 1
            or not hip.lib().otp_conv_embd_supported(b, cin, h, w, cout, ks)):
        raise ValueError(f"conv_embd: kernel size must be one of {CONV_EMBD_KS} and 1 <= channels <= {CONV_EMBD_MAX_CHANNELS}, got "
                         f"ks {ks}, {cin} -> {cout} channels on a ({b}, {cin}, {h}, {w}) input")


def pack_conv_embd_weight(weight):
    """(Cout, Cin, ks, ks) -> the packed [tap][Cin4][CoutP] device tensor of :func:`conv_embd` (csrc/convembd.hip)."""
    _require_gpu(weight)
    _check_f32(weight)
    w = _f32(weight)
    if w.dim() != 4 or w.shape[2] != w.shape[3]:
        raise ValueError(f"conv_embd: weight must be (Cout, Cin, ks, ks), got {tuple(weight.shape)}")
    cout, cin, ks, _ = w.shape
    L = hip.lib()
    nbytes = L.otp_conv_embd_weight_bytes(cin, cout, ks)
    if nbytes == 0:
        check_conv_embd(1, cin, 1, 1, cout, ks)
    wp = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    _launch(L.otp_conv_embd_pack_weight, "otp_conv_embd_pack_weight", (hip.ptr(w), hip.ptr(wp), cin, cout, ks), w)
    return wp


def conv_embd_params(x_shape, weight, bias, ln_weight, ln_bias, pe, device):
    """The checked, flattened fp32 forms (bias, gamma, beta, pe) of a conv embedding layer's optional arguments for an input of
    ``x_shape`` (B, Cin, H, W): ``ValueError`` for anything that does not fit."""
    if len(x_shape) != 4 or weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise ValueError(f"conv_embd: x must be (B, Cin, H, W) and weight (Cout, Cin, ks, ks), got {tuple(x_shape)} and "
                         f"{tuple(weight.shape)}")
    b, cin, h, w = x_shape
    cout, cin_w, ks, _ = weight.shape
    if cin_w != cin:
        raise ValueError(f"conv_embd: weight takes {cin_w} input channels, x has {cin}")
    check_conv_embd(b, cin, h, w, cout, int(ks))
    if (ln_weight is None) != (ln_bias is None):
        raise ValueError("conv_embd: ln_weight and ln_bias come together (both or neither)")
    flat = []
    for name, t in (("bias", bias), ("ln_weight", ln_weight), ("ln_bias", ln_bias)):
        if t is not None and t.numel() != cout:
            raise ValueError(f"conv_embd: {name} has {t.numel()} entries, the layer has {cout} output channels")
        flat.append(None if t is None else _f32(t, device).reshape(cout))
    if pe is not None:
        if pe.numel() != cout * h * w:
            raise ValueError(f"conv_embd: pe must hold ({cout}, {h * w}) entries, got {tuple(pe.shape)}")
        pe = _f32(pe, device).reshape(cout, h * w)
    return (*flat, pe)


def conv_embd_args(x, wpacked, bias, gamma, beta, pe, out, z, cout, ks, eps):
    b, cin, h, w = x.shape
    return (hip.ptr(x), hip.ptr(wpacked), hip.ptr(bias), hip.ptr(gamma), hip.ptr(beta), hip.ptr(pe), hip.ptr(out), hip.ptr(z),
            b, cin, h, w, cout, int(ks), float(eps))


def conv_embd(x, weight, bias, ln_weight, ln_bias, pe=None, eps=1e-5):
    """One conv embedding layer of ConvTransformer (ConvVideoTransformer.py:60-78, 129-135) as one launch in exact fp32:
    ``relu(LayerNorm_c(conv2d(x, weight, bias, padding=ks // 2))) (+ pe)`` on x (B, Cin, H, W) -> (B, Cout, H * W).  ``ln_weight`` /
    ``ln_bias`` ((1, Cout, 1) or None: no norm) are the channel LayerNorm of model/blocks.py:95-110, ``pe`` (Cout, H * W) is
    added behind the ReLU."""
    _require_gpu(x, weight)
    _check_f32(x, weight)
    x = x.contiguous()
    bias, gamma, beta, pe = conv_embd_params(x.shape, weight, bias, ln_weight, ln_bias, pe, x.device)
    cout, ks = weight.shape[0], weight.shape[2]
    out = torch.empty((x.shape[0], cout, x.shape[2] * x.shape[3]), dtype=torch.float32, device=x.device)
    _launch(hip.lib().otp_conv_embd, "otp_conv_embd",
            conv_embd_args(x, pack_conv_embd_weight(weight), bias, gamma, beta, pe, out, None, cout, ks, eps), x)
    return out


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
    _require_gpu(f, w1, w2)
    _check_f32(f, w1, w2)
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
    _require_gpu(f, gate_c, w31, w32)
    _check_f32(f, gate_c, w31, w32)
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
    _require_gpu(x)
    _check_f32(x)
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


def upsample_linear_args(x, out, f, out_coff=0):
    """``x`` (B, C, T) or (B, C, H, W) with T = H * W, written to channels [out_coff, out_coff + C) of ``out``."""
    b, c = x.shape[:2]
    return (hip.ptr(x), hip.ptr(out), b, c, x.numel() // (b * c), f, out.shape[1], out_coff)


def upsample_linear(x, f, out=None, out_coff=0):
    _require_gpu(x)
    b, c, t = x.shape
    if out is None:
        out = torch.empty((b, c, t * f), dtype=x.dtype, device=x.device)
    _launch(hip.lib().otp_upsample_linear, "otp_upsample_linear", upsample_linear_args(x, out, f, out_coff), x)
    return out


def get_max_preds(batch_heatmaps):
    """Device form of reference utils/heatmap.py:143-171: (N,J,H,W) heat-maps -> (preds (N,J,2), maxvals (N,J,1)),
    no device-to-host copy of the maps."""
    return _decode(batch_heatmaps, None, None, refine=False)


def get_final_preds(batch_heatmaps, center=None, scale=None):
    """Device form of reference utils/heatmap.py:108-132: argmax, +-0.25 px shift towards the higher neighbour, and
    (when ``center`` / ``scale`` (N,2) are given) the rot = 0 inverse crop transform of transform_preds."""
    return _decode(batch_heatmaps, center, scale, refine=True)


def _decode(hm, center, scale, refine):
    _require_gpu(hm)
    _check_f32(hm)
    if hm.dim() != 4:
        raise AssertionError("batch_images should be 4-ndim")
    hm = hm.contiguous()
    n, j, h, w = hm.shape
    preds = torch.empty((n, j, 2), dtype=torch.float32, device=hm.device)
    maxvals = torch.empty((n, j, 1), dtype=torch.float32, device=hm.device)
    c = s_ = None
    if center is not None:
        c = torch.as_tensor(center, dtype=torch.float32, device=hm.device).reshape(n, 2).contiguous()
        s_ = torch.as_tensor(scale, dtype=torch.float32, device=hm.device).reshape(n, 2).contiguous()
    hip.check(hip.lib().otp_heatmap_decode(hip.ptr(hm), hip.ptr(preds), hip.ptr(maxvals), hip.ptr(c), hip.ptr(s_),
                                           n, j, h, w, int(refine), hip.stream_of(hm)), "otp_heatmap_decode")
    return preds, maxvals


def flip_permutation(pairs, num_joints):
    """The involution of the left/right ``pairs`` over ``num_joints`` joints as an int32 numpy array (unpaired joints map
    to themselves) - what HRNet's ``flip_back`` swaps.  Host only; raises ``ValueError`` for a joint outside
    [0, num_joints) or one that appears twice (the pairs would not be an involution)."""
    import numpy as np
    j = int(num_joints)
    if j <= 0:
        raise ValueError("num_joints must be positive")
    perm = np.arange(j, dtype=np.int32)
    seen = set()
    for pair in pairs:
        if len(pair) != 2:
            raise ValueError(f"flip pair {pair!r} is not a pair")
        a, b = (int(v) for v in pair)
        for v in (a, b):
            if not 0 <= v < j:
                raise ValueError(f"flip pair {pair!r}: joint {v} outside [0, {j})")
            if v in seen:
                raise ValueError(f"flip pairs: joint {v} appears twice (not an involution)")
            seen.add(v)
        perm[a], perm[b] = b, a
    return perm


def flip_test_merge(hm_pair, flip_pairs=FLIP_PAIRS, shift_heatmap=False, center=None, scale=None):
    """Flip test of HRNet's ``validate`` (TEST.FLIP_TEST / TEST.SHIFT_HEATMAP) in one kernel: ``hm_pair`` (2B, J, H, W)
    float32 are the heat-maps of one forward over the plain clips ``[:B]`` and their mirrors ``[B:]`` (:func:`mirror_pair`,
    ``crop_clips(mirror_pair=True)``).  The mirrored maps are flipped back with the left/right joints of ``flip_pairs``
    (``augment.FLIP_PAIRS``: PoseTrack's 17 joints) swapped, shifted one column right under ``shift_heatmap``, and averaged with the plain
    maps as ``(a + b) * 0.5`` in float32; ``get_final_preds`` of the result comes out of the same pass.  Returns
    ``(merged (B, J, H, W), preds (B, J, 2), maxvals (B, J, 1))``; ``center`` / ``scale`` (B, 2) as for
    :func:`get_final_preds`."""
    _require_gpu(hm_pair)
    _check_f32(hm_pair)
    if hm_pair.dim() != 4 or hm_pair.shape[0] % 2:
        raise ValueError("hm_pair must be a (2B, J, H, W) tensor")
    hm_pair = hm_pair.contiguous()
    n2, j, h, w = hm_pair.shape
    n = n2 // 2
    perm = flip_permutation(flip_pairs, j)
    merged = torch.empty((n, j, h, w), dtype=torch.float32, device=hm_pair.device)
    preds = torch.empty((n, j, 2), dtype=torch.float32, device=hm_pair.device)
    maxvals = torch.empty((n, j, 1), dtype=torch.float32, device=hm_pair.device)
    c = s_ = None
    if (center is None) != (scale is None):
        raise ValueError("center and scale go together")
    if center is not None:
        c = torch.as_tensor(center, dtype=torch.float32, device=hm_pair.device).reshape(n, 2).contiguous()
        s_ = torch.as_tensor(scale, dtype=torch.float32, device=hm_pair.device).reshape(n, 2).contiguous()
    hip.check(hip.lib().otp_heatmap_flip_decode(hip.ptr(hm_pair), perm.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), hip.ptr(merged),
                                                hip.ptr(preds), hip.ptr(maxvals), hip.ptr(c), hip.ptr(s_), n, j, h, w,
                                                int(bool(shift_heatmap)), hip.stream_of(hm_pair)),
              "otp_heatmap_flip_decode")
    return merged, preds, maxvals


def mirror_pair(x, out=None):
    """The flip-test twin batch of clips that are already normalised: ``x`` (B, C, H, W) float32 -> (2B, C, H, W) with
    ``[:B] = x`` and ``[B:] = x.flip(3)`` (script/Common.py:348-354), one streaming kernel.  ``out`` is written in place."""
    _require_gpu(x)
    _check_f32(x)
    if x.dim() != 4:
        raise ValueError("x must be a (B, C, H, W) tensor")
    x = x.contiguous()
    b, c, h, w = x.shape
    if out is None:
        out = torch.empty((2 * b, c, h, w), dtype=torch.float32, device=x.device)
    elif (tuple(out.shape) != (2 * b, c, h, w) or out.dtype != torch.float32 or not out.is_contiguous()
          or out.device != x.device):
        raise ValueError("out must be a contiguous float32 (2B, C, H, W) tensor on x's device")
    hip.check(hip.lib().otp_clip_mirror_pair(hip.ptr(x), hip.ptr(out), b, c, h, w, hip.stream_of(x)),
              "otp_clip_mirror_pair")
    return out


def accuracy(output, target, hm_type="gaussian", thr=0.5):
    """Device form of reference utils/evaluate.py:384-415 (called per iteration at script/Common.py:147-150 on heat-maps
    copied to the host): PCK of the argmax of ``output`` against the argmax of ``target``.  Returns
    ``(acc (J+1), avg_acc, cnt, pred)`` like the reference, as device tensors (no synchronisation)."""
    if hm_type != "gaussian":
        raise NotImplementedError("only hm_type='gaussian' (the reference's only caller)")
    pred, _ = get_max_preds(output)
    tgt, _ = get_max_preds(target)
    n, j, h, w = output.shape
    acc = torch.empty(j + 1, dtype=torch.float32, device=output.device)
    cnt = torch.empty(1, dtype=torch.int32, device=output.device)
    hip.check(hip.lib().otp_pck_accuracy(hip.ptr(pred), hip.ptr(tgt), hip.ptr(acc), hip.ptr(cnt), n, j, h, w, float(thr),
                                         hip.stream_of(output)), "otp_pck_accuracy")
    return acc, acc[0], cnt[0], pred


POSEVAL_JOINTS, POSEVAL_MAX_PR, POSEVAL_MAX_GT = _K["OTP_POSEVAL_JOINTS"], _K["OTP_POSEVAL_MAX_PR"], _K["OTP_POSEVAL_MAX_GT"]


def _poseval_arg(t, dtype, shape, name):
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise TypeError(f"{name} must be a {dtype} tensor")
    _require_gpu(t)
    if t.dim() != len(shape) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
        raise ValueError(f"{name} must have shape {tuple('*' if s is None else s for s in shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def pose_assign(pr_off, pr_sample, preds, maxvals, box_score, gt_off, gt_xy, gt_has, gt_head, poly_off, vert_off, vert_xy,
                dist_thresh=0.5):
    """Device form of reference utils/evaluate.py:22-67 + 467-682 (removeIgnoredPoints, assignGTmulti) over CSR-packed
    frames, one launch (``otp_pose_assign``; layout in include/otpose_hip.h, packing in ``posetrack_eval``).  Returns
    ``(labels (NP,15) int8, scores (NP,15) float64, ngt (F,15) int32)``: label 1 match, 0 false positive, -1 no entry.
    Raises ``ValueError`` for a frame with more than ``POSEVAL_MAX_PR`` predicted or ``POSEVAL_MAX_GT`` ground-truth
    persons or a sample index outside ``preds`` (the offsets are read back for the check: this is evaluation plumbing, it
    synchronises)."""
    i32, f64 = torch.int32, torch.float64
    pr_off = _poseval_arg(pr_off, i32, (None,), "pr_off")
    f = pr_off.numel() - 1
    pr_sample = _poseval_arg(pr_sample, i32, (None,), "pr_sample")
    preds = _poseval_arg(preds, torch.float32, (None, 17, 2), "preds")
    n = preds.shape[0]
    if torch.is_tensor(maxvals) and maxvals.dim() == 2:
        maxvals = maxvals.unsqueeze(-1)
    maxvals = _poseval_arg(maxvals, torch.float32, (n, 17, 1), "maxvals")
    box_score = _poseval_arg(box_score, f64, (n,), "box_score")
    gt_off = _poseval_arg(gt_off, i32, (f + 1,), "gt_off")
    gt_xy = _poseval_arg(gt_xy, f64, (None, POSEVAL_JOINTS, 2), "gt_xy")
    ng = gt_xy.shape[0]
    gt_has = _poseval_arg(gt_has, i32, (ng,), "gt_has")
    gt_head = _poseval_arg(gt_head, f64, (ng, 4), "gt_head")
    poly_off = _poseval_arg(poly_off, i32, (f + 1,), "poly_off")
    vert_off = _poseval_arg(vert_off, i32, (None,), "vert_off")
    vert_xy = _poseval_arg(vert_xy, f64, (None, 2), "vert_xy")
    npr = pr_sample.numel()
    if f <= 0 or npr <= 0:
        raise ValueError("pose_assign needs at least one frame and one predicted person")
    if vert_off.numel() < 1:
        raise ValueError("vert_off must hold at least its leading 0")
    checks = torch.stack([
        (pr_off[1:] - pr_off[:-1]).max(), (pr_off[1:] - pr_off[:-1]).min(), pr_off[0], pr_off[-1],
        (gt_off[1:] - gt_off[:-1]).max(), (gt_off[1:] - gt_off[:-1]).min(), gt_off[0], gt_off[-1],
        (poly_off[1:] - poly_off[:-1]).min(), poly_off[0], poly_off[-1],
        pr_sample.max(), pr_sample.min(),
        (vert_off[1:] - vert_off[:-1]).min() if vert_off.numel() > 1 else vert_off[0] * 0, vert_off[0], vert_off[-1],
    ]).tolist()
    (pmax, pmin, pfirst, plast, gmax, gmin, gfirst, glast, qmin, qfirst, qlast, smax, smin, vmin, vfirst, vlast) = checks
    if pmax > POSEVAL_MAX_PR:
        raise ValueError(f"a frame has {pmax} predicted persons, the kernel's limit is {POSEVAL_MAX_PR}")
    if gmax > POSEVAL_MAX_GT:
        raise ValueError(f"a frame has {gmax} ground-truth persons, the kernel's limit is {POSEVAL_MAX_GT}")
    if (pmin < 0 or pfirst != 0 or plast != npr or gmin < 0 or gfirst != 0 or glast != ng or qmin < 0 or qfirst != 0
            or qlast != vert_off.numel() - 1 or vmin < 0 or vfirst != 0 or vlast != vert_xy.shape[0]):
        raise ValueError("inconsistent CSR offsets")
    if smax >= n or smin < -1:
        raise ValueError(f"pr_sample outside [-1, {n})")
    labels = torch.empty((npr, POSEVAL_JOINTS), dtype=torch.int8, device=pr_off.device)
    scores = torch.empty((npr, POSEVAL_JOINTS), dtype=f64, device=pr_off.device)
    ngt = torch.empty((f, POSEVAL_JOINTS), dtype=i32, device=pr_off.device)
    hip.check(hip.lib().otp_pose_assign(
        hip.ptr(pr_off), hip.ptr(pr_sample), hip.ptr(preds), hip.ptr(maxvals), hip.ptr(box_score), hip.ptr(gt_off),
        hip.ptr(gt_xy), hip.ptr(gt_has), hip.ptr(gt_head), hip.ptr(poly_off), hip.ptr(vert_off), hip.ptr(vert_xy),
        float(dist_thresh), hip.ptr(labels), hip.ptr(scores), hip.ptr(ngt), f, npr, n, ng, hip.stream_of(pr_off)),
        "otp_pose_assign")
    return labels, scores, ngt


def sort_entries(labels, scores):
    """The torch plumbing between :func:`pose_assign` and :func:`ap_curve`: per joint, drop the -1 entries and order the
    rest by DESCENDING score, ties in the order a stable ascending sort followed by a reversal gives (of two entries with
    the same score, the one of the later person comes first).  Returns ``(labels_sorted (E,) int8, joint_off (J+1,) int64,
    scores_sorted (E,) float64)``, the joints concatenated."""
    lab = labels.t().contiguous()                                    # (J, NP)
    order = torch.sort(scores.t().contiguous(), dim=1, stable=True).indices.flip(1)
    lab = torch.gather(lab, 1, order)
    sc = torch.gather(scores.t(), 1, order)
    keep = lab >= 0
    joint_off = torch.zeros(lab.shape[0] + 1, dtype=torch.int64, device=lab.device)
    joint_off[1:] = keep.sum(1).cumsum(0)
    return lab[keep], joint_off, sc[keep]


def ap_curve(labels_sorted, joint_off, n_gt, return_curve=False):
    """Device form of reference utils/evaluate.py:686-751 (compute_rpc + vocap) for every joint in one launch
    (``otp_ap_curve``): ``labels_sorted`` (E,) int8 holds the 0 / 1 entries of joint j at ``joint_off[j]:joint_off[j+1]``
    (int64) in descending score order (:func:`sort_entries` states the tie rule), ``n_gt`` (J,) int64 the annotated joints.
    Returns ``out (J,3) float64`` = AP, last precision, last recall, x 100 as compute_metrics reports them (zeros for a
    joint without entries); with ``return_curve`` also the float64 precision and recall of every entry."""
    labels_sorted = _poseval_arg(labels_sorted, torch.int8, (None,), "labels_sorted")
    joint_off = _poseval_arg(joint_off, torch.int64, (None,), "joint_off")
    j = joint_off.numel() - 1
    n_gt = _poseval_arg(n_gt, torch.int64, (j,), "n_gt")
    if j <= 0:
        raise ValueError("ap_curve needs at least one joint")
    first, last, dmin = torch.stack([joint_off[0], joint_off[-1], (joint_off[1:] - joint_off[:-1]).min()]).tolist()
    if first != 0 or last != labels_sorted.numel() or dmin < 0:
        raise ValueError("joint_off does not partition labels_sorted")
    dev = joint_off.device
    out = torch.zeros((j, 3), dtype=torch.float64, device=dev)
    prec = torch.empty(labels_sorted.numel(), dtype=torch.float64, device=dev) if return_curve else None
    rec = torch.empty_like(prec) if return_curve else None
    if labels_sorted.numel():
        hip.check(hip.lib().otp_ap_curve(hip.ptr(labels_sorted), hip.ptr(joint_off), hip.ptr(n_gt), hip.ptr(out),
                                         hip.ptr(prec), hip.ptr(rec), j, hip.stream_of(joint_off)), "otp_ap_curve")
    return (out, prec, rec) if return_curve else out


# COCO's per-joint sigmas (17 joints in the model's order), as HRNet's lib/nms/nms.py carries them
COCO_SIGMAS = tuple(v / 10.0 for v in (.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89))
_SOFT_TYPES = {"gaussian": 1, "linear": 2}


def pose_nms(pr_off, pr_sample, preds, maxvals, box_score, area, *, oks_thresh, in_vis_thre=0.0, oks_in_vis_thre=None,
             sigmas=COCO_SIGMAS, soft=False, soft_type="gaussian", max_dets=20, return_oks=False):
    """Keypoint rescoring and per-frame OKS suppression of top-down predictions over the CSR of :func:`pose_assign`, one
    launch (``otp_pose_nms``; the arithmetic is the contract in include/otpose_hip.h).  ``area`` (N,) float64 is the
    box area of each sample (``prod(scale * 200)`` for a crop).  Returns ``(keep (NP,) bool, person_score (NP,) float64,
    rank (NP,) int32[, oks (NP,64) float64])``: hard NMS gives the rescored person score and the position in the
    descending order, ``soft=True`` (``soft_type`` "gaussian" / "linear", at most ``max_dets`` kept per frame) the decayed
    score and the step at which the person was taken (-1: never).  The placeholder person (-1) is always kept.
    Raises ``ValueError`` for a frame with more than ``POSEVAL_MAX_PR`` persons, inconsistent offsets, a sample index
    outside ``preds`` or a bad setting (the offsets are read back for the check: it synchronises)."""
    i32, f64 = torch.int32, torch.float64
    pr_off = _poseval_arg(pr_off, i32, (None,), "pr_off")
    f = pr_off.numel() - 1
    pr_sample = _poseval_arg(pr_sample, i32, (None,), "pr_sample")
    preds = _poseval_arg(preds, torch.float32, (None, 17, 2), "preds")
    n = preds.shape[0]
    if torch.is_tensor(maxvals) and maxvals.dim() == 2:
        maxvals = maxvals.unsqueeze(-1)
    maxvals = _poseval_arg(maxvals, torch.float32, (n, 17, 1), "maxvals")
    box_score = _poseval_arg(box_score, f64, (n,), "box_score")
    area = _poseval_arg(area, f64, (n,), "area")
    npr = pr_sample.numel()
    if f <= 0 or npr <= 0:
        raise ValueError("pose_nms needs at least one frame and one predicted person")
    sig = [float(s) for s in sigmas]
    if len(sig) != 17 or not all(math.isfinite(s) and s > 0 for s in sig):
        raise ValueError("sigmas must be 17 positive finite numbers")
    oks_thresh = float(oks_thresh)
    if not (math.isfinite(oks_thresh) and oks_thresh > 0):
        raise ValueError("oks_thresh must be finite and positive")
    if int(max_dets) < 1:
        raise ValueError("max_dets must be at least 1")
    if soft and soft_type not in _SOFT_TYPES:
        raise ValueError(f"soft_type must be one of {sorted(_SOFT_TYPES)}")
    pmax, pmin, pfirst, plast, smax, smin = torch.stack([
        (pr_off[1:] - pr_off[:-1]).max(), (pr_off[1:] - pr_off[:-1]).min(), pr_off[0], pr_off[-1],
        pr_sample.max(), pr_sample.min()]).tolist()
    if pmax > POSEVAL_MAX_PR:
        raise ValueError(f"a frame has {pmax} predicted persons, the kernel's limit is {POSEVAL_MAX_PR}")
    if pmin < 0 or pfirst != 0 or plast != npr:
        raise ValueError("inconsistent CSR offsets")
    if smax >= n or smin < -1:
        raise ValueError(f"pr_sample outside [-1, {n})")
    dev = pr_off.device
    keep = torch.empty(npr, dtype=torch.int8, device=dev)
    score = torch.empty(npr, dtype=f64, device=dev)
    rank = torch.empty(npr, dtype=i32, device=dev)
    oks = torch.empty((npr, POSEVAL_MAX_PR), dtype=f64, device=dev) if return_oks else None
    hip.check(hip.lib().otp_pose_nms(
        hip.ptr(pr_off), hip.ptr(pr_sample), hip.ptr(preds), hip.ptr(maxvals), hip.ptr(box_score), hip.ptr(area),
        (ctypes.c_double * 17)(*sig), float(in_vis_thre), oks_thresh,
        math.nan if oks_in_vis_thre is None else float(oks_in_vis_thre), _SOFT_TYPES[soft_type] if soft else 0,
        int(max_dets), hip.ptr(keep), hip.ptr(score), hip.ptr(rank), hip.ptr(oks), f, npr, n, hip.stream_of(pr_off)),
        "otp_pose_nms")
    keep = keep.view(torch.bool)
    return (keep, score, rank, oks) if return_oks else (keep, score, rank)


IMAGENET_MEAN = (0.485, 0.456, 0.406)        # utils/transform.py:7-8
IMAGENET_STD = (0.229, 0.224, 0.225)


def frames_to_clip(frames_u8, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """uint8 RGB frames (B, F, H, W, 3) (the five warped crops of dataset/PoseTrackDataset.py:390-399) -> the model input
    (B, 3F, H, W) float32: ToTensor + Normalize per frame (utils/transform.py:11-15) and the channel concat of
    script/Common.py:117 in one kernel, bit-identical to the torchvision float32 arithmetic.  Moves 4x fewer bytes over
    PCIe than shipping normalised floats."""
    _require_gpu(frames_u8)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 5 or frames_u8.shape[-1] != 3:
        raise TypeError("frames_u8 must be a (B, F, H, W, 3) uint8 tensor")
    frames_u8 = frames_u8.contiguous()
    b, f, h, w, _ = frames_u8.shape
    if out is None:
        out = torch.empty((b, 3 * f, h, w), dtype=torch.float32, device=frames_u8.device)
    elif out.shape != (b, 3 * f, h, w) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 (B, 3F, H, W) tensor")
    hip.check(hip.lib().otp_frames_u8_to_clip(hip.ptr(frames_u8), hip.ptr(out), b, f, h, w, *[float(v) for v in mean],
                                              *[float(v) for v in std], hip.stream_of(frames_u8)),
              "otp_frames_u8_to_clip")
    return out


def _host_or_device(x, dtype, device, name, shape):
    """``x`` (numpy / list / tensor) as a contiguous ``dtype`` tensor on ``device`` of the given shape."""
    t = torch.as_tensor(x)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_cuda and dtype.is_floating_point and not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} has non-finite values")
    return t.to(device=device, dtype=dtype).contiguous()


def crop_clips(pool, frame_idx, M, flip=None, out=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, size=None, blur=None,
               blur_on=None, mirror_pair=False):
    """Person crops straight from whole frames: ``pool`` (S, Hp, Wp, 3) uint8 RGB on the GPU, ``frame_idx`` (B, F) pool
    frame of each window slot, ``M`` (B, 2, 3) float64 forward crop matrices (otpose_amd.crop.crop_matrix), ``flip`` (B)
    optional: mirror the frame first.  Returns the model input (B, 3F, H, W) float32: five cv2.warpAffine(INTER_LINEAR)
    crops per sample (dataset/PoseTrackDataset.py:389-399, bit-identical fixed-point arithmetic) followed by the
    ToTensor + Normalize + concat of :func:`frames_to_clip`, in one kernel.  ``out`` (written in place) or ``size`` =
    (W, H) gives the crop size.  An index outside [0, S) reads as an empty frame (border value 0); host-side indices
    must fit int32.  Frames of different sizes may share a pool zero-padded to (Hp, Wp): the crops are unchanged
    (except under ``flip``, which mirrors the padded width).

    ``blur`` (B, F, 9, 5) float32 (otpose_amd.augment.blur_table per slot) blurs each slot's frame first, as the
    reference's training T.GaussianBlur((5, 9)) does (9 taps along the width, 5 across RGB, rows never mixed; see
    include/otpose_hip.h for the arithmetic); ``blur_on`` (B, F) optional selects the blurred slots (default: all).
    The blur reflects at column Wp - 1, so every frame of the pool must have the pool's width (a zero-padded narrower
    frame would be blurred with its padding), and Wp >= 5.  ``blur=None`` takes the plain kernel.

    ``mirror_pair=True`` cuts the flip-test twin batch: (2B, 3F, H, W) with the plain crops in ``[:B]`` and their exact
    column mirrors in ``[B:]`` (the mirrored network input, ``torch.flip(out[:B], [3])``), from one gather per value.
    It takes no ``flip`` and no ``blur``."""
    _require_gpu(pool)
    if pool.dtype != torch.uint8 or pool.dim() != 4 or pool.shape[-1] != 3:
        raise TypeError("pool must be an (S, Hp, Wp, 3) uint8 tensor")
    pool = pool.contiguous()
    s, hp, wp, _ = pool.shape
    dev = pool.device
    fi = torch.as_tensor(frame_idx)
    if fi.dim() != 2 or fi.dtype.is_floating_point or fi.dtype == torch.bool:
        raise TypeError("frame_idx must be a (B, F) integer array")
    b, f = fi.shape
    if fi.dtype != torch.int32:
        if not fi.is_cuda and fi.numel() and (int(fi.min()) < -2 ** 31 or int(fi.max()) >= 2 ** 31):
            raise ValueError("frame_idx values must fit int32")
        fi = fi.clamp(-1, s)                    # out-of-range stays out of range through the int32 cast
    fi = fi.to(device=dev, dtype=torch.int32).contiguous()
    M = _host_or_device(M, torch.float64, dev, "M", (b, 2, 3))
    if mirror_pair and (flip is not None or blur is not None or blur_on is not None):
        raise ValueError("mirror_pair takes no flip and no blur")
    fl = None if flip is None else _host_or_device(flip, torch.bool, dev, "flip", (b,)).to(torch.uint8)
    nb = 2 * b if mirror_pair else b
    if out is None:
        if size is None:
            raise ValueError("crop_clips needs out= or size=(W, H)")
        w, h = int(size[0]), int(size[1])
        out = torch.empty((nb, 3 * f, h, w), dtype=torch.float32, device=dev)
    else:
        if (out.dim() != 4 or out.shape[:2] != (nb, 3 * f) or out.dtype != torch.float32 or not out.is_contiguous()
                or out.device != dev):
            what = "(2B, 3F, H, W)" if mirror_pair else "(B, 3F, H, W)"
            raise ValueError(f"out must be a contiguous float32 {what} tensor on the pool's device")
        h, w = out.shape[2:]
        if size is not None and (int(size[0]), int(size[1])) != (w, h):
            raise ValueError("size disagrees with out")
    if mirror_pair:
        hip.check(hip.lib().otp_crop_clips_pair_u8(hip.ptr(pool), s, hp, wp, hip.ptr(fi), hip.ptr(M), hip.ptr(out), b, f,
                                                   h, w, *[float(v) for v in mean], *[float(v) for v in std],
                                                   hip.stream_of(pool)), "otp_crop_clips_pair_u8")
        return out
    if blur is None:
        if blur_on is not None:
            raise ValueError("blur_on needs blur")
        hip.check(hip.lib().otp_crop_clips_u8(hip.ptr(pool), s, hp, wp, hip.ptr(fi), hip.ptr(M), hip.ptr(fl),
                                              hip.ptr(out), b, f, h, w, *[float(v) for v in mean],
                                              *[float(v) for v in std], hip.stream_of(pool)), "otp_crop_clips_u8")
        return out
    if wp < 5:
        raise ValueError(f"the blur needs frames at least 5 pixels wide, got {wp}")
    bt = _host_or_device(blur, torch.float32, dev, "blur", (b, f, 9, 5))
    on = None if blur_on is None else _host_or_device(blur_on, torch.bool, dev, "blur_on", (b, f)).to(torch.uint8)
    hip.check(hip.lib().otp_crop_clips_blur_u8(hip.ptr(pool), s, hp, wp, hip.ptr(fi), hip.ptr(M), hip.ptr(fl),
                                               hip.ptr(out), b, f, h, w, *[float(v) for v in mean],
                                               *[float(v) for v in std], hip.ptr(bt), hip.ptr(on),
                                               hip.stream_of(pool)), "otp_crop_clips_blur_u8")
    return out


_GAUSS = {}            # (sigma, device) -> device copy of the host-built Gaussian patch


def pose_targets(joints, vis, M, sigma, image_size, heatmap_size):
    """Training targets of dataset/PoseTrackDataset.py:403-420 on the GPU: ``joints`` (B, J, 2 or 3) image coordinates,
    ``vis`` (B, J) (or (B, J, 3): column 0 is used), ``M`` (B, 2, 3) the crop matrices of :func:`crop_clips`.  Visible
    joints are moved into the crop, joints outside [0, W] x [0, H] lose their visibility, and generate_heatmaps
    (utils/heatmap.py:48-105) draws the Gaussian patches.  Returns ``(target (B, J, h, w), target_weight (B, J, 1))``
    float32; ``image_size`` = (W, H), ``heatmap_size`` = (w, h), ``sigma`` a whole number."""
    from .crop import gaussian_table
    j = torch.as_tensor(joints, dtype=torch.float64)
    dev = j.device if j.is_cuda else torch.as_tensor(M).device
    if dev.type != "cuda":
        raise NotImplementedError("pose_targets runs on the GPU only: pass joints or M as a GPU tensor")
    gaussian_table(sigma)                      # validates sigma
    if j.dim() != 3 or j.shape[-1] not in (2, 3):
        raise ValueError("joints must be (B, J, 2) or (B, J, 3)")
    b, nj = j.shape[:2]
    j = j[..., :2].to(dev).contiguous()
    v = torch.as_tensor(vis)
    v = (v[..., 0] if v.dim() == 3 else v).to(device=dev, dtype=torch.float32).contiguous()
    if tuple(v.shape) != (b, nj):
        raise ValueError("vis must be (B, J) or (B, J, 3)")
    M = _host_or_device(M, torch.float64, dev, "M", (b, 2, 3))
    key = (int(sigma), dev)
    if key not in _GAUSS:
        _GAUSS[key] = torch.from_numpy(gaussian_table(sigma)).to(dev)
    W, H = int(image_size[0]), int(image_size[1])
    w, h = int(heatmap_size[0]), int(heatmap_size[1])
    target = torch.empty((b, nj, h, w), dtype=torch.float32, device=dev)
    weight = torch.empty((b, nj, 1), dtype=torch.float32, device=dev)
    hip.check(hip.lib().otp_pose_targets(hip.ptr(j), hip.ptr(v), hip.ptr(M), hip.ptr(_GAUSS[key]), hip.ptr(target),
                                         hip.ptr(weight), b, nj, W, H, w, h, 3 * int(sigma), hip.stream_of(target)),
              "otp_pose_targets")
    return target, weight


PosePlan = collections.namedtuple("PosePlan", "center scale M frame_idx margin box_score person_slot pr_off total")


def _plan_arg(t, dtype, shape, name):
    """One device input of :func:`pose_plan`: type, then shape, then device (so every argument error shows without a GPU)."""
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise TypeError(f"{name} must be a {dtype} tensor")
    if t.dim() != len(shape) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
        raise ValueError(f"{name} must have shape {tuple('*' if s is None else s for s in shape)}, got {tuple(t.shape)}")
    return t


def pose_plan(boxes, scores, counts, frame_number, num_frames, *, image_size, max_persons, detect=None, min_score=0.0,
              enlarge=1.25, posetrack18=True, aspect_ratio=None, window_frames=5):
    """The crop plan of the video path, on the device in one launch (``otp_pose_plan``, csrc/plan.hip): what
    ``crop.box_to_center_scale``, ``crop.crop_matrix`` (rotation 0) and ``crop.window`` compute per person on the host,
    plus the compaction of the detector's (frame, box) grid into dense rows in (frame, box) order.

    ``boxes`` (S, K, 4) float64 ``x, y, w, h``, ``scores`` (S, K) float32 and ``counts`` (S) int32 are
    ``PersonDetector.detect``'s device output over the pool; ``frame_number`` (S) int32 is each pool frame's number as in
    the file name and ``num_frames`` (S) int32 the length of its sequence (per frame: one pool may hold several videos,
    each as a run of consecutive frame numbers).  Only slots in ``detect = (lo, hi)`` (default: all) yield persons, the
    others are the halo the windows read; boxes scoring below ``min_score`` are dropped.  ``image_size`` = (W, H) is
    ``MODEL.IMAGE_SIZE`` (the crop size; ``aspect_ratio`` defaults to W / H), ``enlarge`` the box enlargement.

    Returns a :class:`PosePlan` of device tensors with ``P = max_persons`` rows: ``center`` / ``scale`` (P, 2) float32,
    ``M`` (P, 2, 3) float64, ``frame_idx`` (P, 5) int32 pool slots (cur, prev, next, pprev, nnext; -1: an empty frame),
    ``margin`` (P, 4) float32, ``box_score`` (P) float64, ``person_slot`` (P) int32, ``pr_off`` (S + 1) int32 per-frame
    row offsets (capped at P) and ``total`` (1) int32: the persons kept, NOT capped - rows past ``min(total, P)`` are
    padding (identity ``M``, ``frame_idx`` -1, the rest 0 / -1).  Nothing is read back: ``int(plan.total)`` is the caller's
    one synchronisation."""
    if int(window_frames) != 5:
        raise ValueError(f"pose_plan builds the 5-frame window of crop.window, not {window_frames} frames")
    i32 = torch.int32
    boxes = _plan_arg(boxes, torch.float64, (None, None, 4), "boxes")
    s, k = boxes.shape[:2]
    scores = _plan_arg(scores, torch.float32, (s, k), "scores")
    counts = _plan_arg(counts, i32, (s,), "counts")
    frame_number = _plan_arg(frame_number, i32, (s,), "frame_number")
    num_frames = _plan_arg(num_frames, i32, (s,), "num_frames")
    if s < 1:
        raise ValueError("pose_plan needs at least one pool frame")
    lo, hi = (0, s) if detect is None else (int(detect[0]), int(detect[1]))
    if not 0 <= lo <= hi <= s:
        raise ValueError(f"detect = ({lo}, {hi}) is not a range of the {s} pool frames")
    w_img, h_img = int(image_size[0]), int(image_size[1])
    if w_img < 1 or h_img < 1:
        raise ValueError("image_size must be (W, H) with both positive")
    ar = w_img * 1.0 / h_img if aspect_ratio is None else float(aspect_ratio)
    min_score, enlarge, p = float(min_score), float(enlarge), int(max_persons)
    if not (math.isfinite(ar) and ar > 0 and math.isfinite(enlarge) and enlarge > 0) or math.isnan(min_score):
        raise ValueError("aspect_ratio and enlarge must be positive and finite, min_score a number")
    if p < 0:
        raise ValueError("max_persons must not be negative")
    tensors = (boxes, scores, counts, frame_number, num_frames)
    _require_gpu(*tensors)
    dev = boxes.device
    if any(t.device != dev for t in tensors):
        raise ValueError("pose_plan's inputs must share one device")
    boxes, scores, counts, frame_number, num_frames = (t.contiguous() for t in tensors)
    f32, f64 = torch.float32, torch.float64
    plan = PosePlan(torch.empty((p, 2), dtype=f32, device=dev), torch.empty((p, 2), dtype=f32, device=dev),
                    torch.empty((p, 2, 3), dtype=f64, device=dev), torch.empty((p, 5), dtype=i32, device=dev),
                    torch.empty((p, 4), dtype=f32, device=dev), torch.empty((p,), dtype=f64, device=dev),
                    torch.empty((p,), dtype=i32, device=dev), torch.empty((s + 1,), dtype=i32, device=dev),
                    torch.empty((1,), dtype=i32, device=dev))
    hip.check(hip.lib().otp_pose_plan(
        hip.ptr(boxes), hip.ptr(scores), hip.ptr(counts), hip.ptr(frame_number), hip.ptr(num_frames), s, k, lo, hi, min_score,
        ar, enlarge, w_img, h_img, int(bool(posetrack18)), p, *[hip.ptr(t) for t in plan], hip.stream_of(boxes)),
        "otp_pose_plan")
    return plan


def st_ohkw_loss(s, t, g, w, topk=8, flags=None, with_grad=False):
    """ST_OHKW_MSELoss forward (+ analytic gradients) on the GPU; returns dict like the reference
    (model/loss.py:89-91) plus ``flags`` and, when requested, ``grad_s`` / ``grad_t``."""
    _require_gpu(s, t, g, w)
    b, j = s.shape[:2]
    hw = s[0, 0].numel()
    s, t, g = s.contiguous(), t.contiguous(), g.contiguous()
    wv = w.reshape(b, j).contiguous().float()
    L = hip.lib()
    nbytes = L.otp_loss_workspace(b, j)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=s.device)
    res = torch.empty(3, dtype=torch.float32, device=s.device)
    given = flags is not None
    fl = flags.to(torch.int32).contiguous() if given else torch.empty(j, dtype=torch.int32, device=s.device)
    gs = torch.empty_like(s) if with_grad else None
    gt = torch.empty_like(t) if with_grad else None
    hip.check(L.otp_loss_st_ohkw(hip.ptr(s), hip.ptr(t), hip.ptr(g), hip.ptr(wv), hip.ptr(fl), hip.ptr(res),
                                 hip.ptr(gs), hip.ptr(gt), hip.ptr(ws), nbytes, b, j, hw, topk, int(given),
                                 hip.stream_of(s)), "otp_loss_st_ohkw")
    out = {"ohkm_loss_s": res[0], "mse_loss_s": res[1], "final_loss": res[2], "flags": fl}
    if with_grad:
        out["grad_s"], out["grad_t"] = gs, gt
    return out


def _joints_mse(o, g, w, topk, ohkm, effective_num_joints, with_grad):
    _require_gpu(o, g)
    b, j = o.shape[:2]
    hw = o[0, 0].numel()
    o, g = o.contiguous(), g.contiguous()
    wv = None if w is None else w.reshape(b, j).contiguous().float()
    L = hip.lib()
    nbytes = L.otp_loss_workspace(b, j)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=o.device)
    res = torch.empty(3, dtype=torch.float32, device=o.device)
    go = torch.empty_like(o) if with_grad else None
    hip.check(L.otp_loss_joints_mse(hip.ptr(o), hip.ptr(g), hip.ptr(wv), hip.ptr(res), hip.ptr(go), hip.ptr(ws), nbytes,
                                    b, j, hw, topk, int(ohkm), int(effective_num_joints or 0), hip.stream_of(o)),
              "otp_loss_joints_mse")
    return res, go


def joints_ohkm_mse_loss(output, target, target_weight=None, effective_num_joints=None, topk=8, with_grad=False):
    """JointsMSE_OHKMMSELoss.forward (model/loss.py:115-148) on the GPU; ``target_weight=None`` is the reference's
    ``use_target_weight=False``.  Returns the reference's dict (+ ``grad_output`` of ``final_loss`` when requested)."""
    res, go = _joints_mse(output, target, target_weight, topk, True, effective_num_joints, with_grad)
    out = {"ohkm_loss": res[0], "mse_loss": res[1], "final_loss": res[2]}
    if with_grad:
        out["grad_output"] = go
    return out


def joint_mse_loss(output, target, target_weight=None, effective_num_joints=None, with_grad=False):
    """JointMSELoss.forward (model/loss.py:158-182) on the GPU: a scalar (and its gradient when requested)."""
    res, go = _joints_mse(output, target, target_weight, 1, False, effective_num_joints, with_grad)
    return (res[2], go) if with_grad else res[2]


# ---- flow-encoder TransformerBlock (C = 17) as two launches around the channel attention (csrc/flowenc.hip) ---------------
def flow_block_supported(blk, c, t) -> bool:
    """Stride-1 TransformerBlock with 17 channels, biases everywhere and one epsilon for ln1 and the q / k / v norms."""
    a = blk.attn
    try:
        eps = {float(m.eps) for m in (blk.ln1, a.query_norm, a.key_norm, a.value_norm)}
        has_bias = all(m.bias is not None for m in (a.query, a.key, a.value, a.proj, blk.mlp[0], blk.mlp[3]))
        dw_ok = all(tuple(m.weight.shape) == (c, 1, 3) and m.bias is None for m in (a.query_conv, a.key_conv, a.value_conv))
    except AttributeError:
        return False
    return (len(eps) == 1 and has_bias and dw_ok
            and bool(hip.lib().otp_flow_block_supported(int(c), int(blk.mlp[0].out_channels), int(t))))


def pack_flow_front(blk, device):
    """Parameter block of ``otp_flow_front`` (layout: include/otpose_hip.h) from a TransformerBlock's modules."""
    a = blk.attn
    f = lambda t: t.detach().to(device, torch.float32).reshape(-1)                     # noqa: E731
    parts = [f(blk.ln1.weight), f(blk.ln1.bias)]
    for conv, norm, proj in ((a.query_conv, a.query_norm, a.query), (a.key_conv, a.key_norm, a.key),
                             (a.value_conv, a.value_norm, a.value)):
        parts += [f(conv.weight), f(norm.weight), f(norm.bias), f(proj.weight), f(proj.bias)]
    prm = torch.cat(parts).contiguous()
    c = blk.ln1.weight.numel()
    assert prm.numel() == hip.lib().otp_flow_front_param_floats(c), (prm.numel(), c)
    return prm


def pack_flow_back(blk, device):
    """Parameter block of ``otp_flow_back``: the drop-path scales (model/blocks.py:298-301, eval: plain per-channel factors)
    folded into the projection / down-projection rows and biases; W_2 transposed to (hidden, C)."""
    a = blk.attn
    d = lambda t: t.detach().to(device, torch.float32)                                 # noqa: E731
    c = blk.ln1.weight.numel()
    hid = blk.mlp[0].out_channels
    sa, sm = d(blk.drop_path_attn.scale).reshape(-1), d(blk.drop_path_mlp.scale).reshape(-1)
    wp = d(a.proj.weight).reshape(c, c) * sa[:, None]
    w2 = d(blk.mlp[3].weight).reshape(c, hid) * sm[:, None]
    parts = [wp.reshape(-1), d(a.proj.bias) * sa, d(blk.ln2.weight).reshape(-1), d(blk.ln2.bias).reshape(-1),
             d(blk.mlp[0].weight).reshape(-1), d(blk.mlp[0].bias), w2.t().contiguous().reshape(-1), d(blk.mlp[3].bias) * sm]
    prm = torch.cat(parts).contiguous()
    assert prm.numel() == hip.lib().otp_flow_back_param_floats(c, hid), (prm.numel(), c, hid)
    return prm


def flow_front_args(x, prm, q, k, v, eps):
    b, c, t = x.shape
    return (hip.ptr(x), hip.ptr(prm), hip.ptr(q), hip.ptr(k), hip.ptr(v), b, c, t, float(eps))


def flow_back_args(x, att, prm, out, hidden, eps):
    b, c, t = x.shape
    return (hip.ptr(x), hip.ptr(att), hip.ptr(prm), hip.ptr(out), b, c, int(hidden), t, float(eps))


def flow_front(x, prm, eps=1e-5):
    """q, k, v of a flow-encoder block from its input (B, 17, T)."""
    _require_gpu(x, prm)
    _check_f32(x)
    x = x.contiguous()
    q, k, v = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    _launch(hip.lib().otp_flow_front, "otp_flow_front", flow_front_args(x, prm, q, k, v, eps), x)
    return q, k, v


def flow_back(x, att, prm, hidden, eps=1e-5):
    """Block output from its input ``x`` and the attention output ``att`` (both (B, 17, T))."""
    _require_gpu(x, att, prm)
    _check_f32(x)
    x, att = x.contiguous(), att.contiguous()
    out = torch.empty_like(x)
    _launch(hip.lib().otp_flow_back, "otp_flow_back", flow_back_args(x, att, prm, out, hidden, eps), x)
    return out


# ---- fp16-storage eval kernels of the backbone (csrc/h16.hip; cfg.MODEL.DTYPE = "fp16") ------------------------------------
class H8:
    """An H8 image: ``t`` = int32 storage of [N][gtot][H * W] 16-byte records (8 halves = channels 8 g .. 8 g + 7 of a pixel),
    of which this tensor is the channel groups [goff, goff + C / 8) - the fp16 engine's activation format (include/otpose_hip.h)."""

    __slots__ = ("t", "N", "C", "H", "W", "gtot", "goff")

    def __init__(self, t, n, c, h, w, gtot=None, goff=0):
        assert c % 8 == 0
        self.t, self.N, self.C, self.H, self.W = t, n, c, h, w
        self.gtot, self.goff = (c // 8 if gtot is None else gtot), goff
        assert 0 <= self.goff and self.goff + c // 8 <= self.gtot

    def slice(self, coff, c):
        assert coff % 8 == 0 and c % 8 == 0 and coff + c <= self.C
        return H8(self.t, self.N, c, self.H, self.W, self.gtot, self.goff + coff // 8)


def h8_empty(n, c, h, w, device):
    nbytes = hip.lib().otp_h8_bytes(n, c, h, w)
    if not nbytes:
        raise ValueError(f"H8 images need a channel count that is a multiple of 8, got {c}")
    return H8(torch.empty(nbytes // 4, dtype=torch.int32, device=device), n, c, h, w)


def h8_pack(x, out: H8 = None, stream=None):
    """fp32 NCHW tensor or channel-slice :class:`View` -> H8 (one rounding to half per element)."""
    iv = x if isinstance(x, View) else View(x.contiguous())
    _require_gpu(iv.t)
    n, _, h, w = iv.t.shape
    out = h8_empty(n, iv.C, h, w, iv.t.device) if out is None else out
    hip.check(hip.lib().otp_h8_pack(hip.ptr(iv.t), hip.ptr(out.t), n, iv.C, h, w, iv.ctot, iv.coff, out.gtot, out.goff,
                                    stream if stream is not None else hip.stream_of(iv.t)), "otp_h8_pack")
    return out


def h8_unpack(img: H8, stream=None):
    """H8 image -> fp32 (N, C, H, W), exact."""
    out = torch.empty(img.N, img.C, img.H, img.W, dtype=torch.float32, device=img.t.device)
    hip.check(hip.lib().otp_h8_unpack(hip.ptr(img.t), hip.ptr(out), img.N, img.C, img.H, img.W, img.gtot, img.goff,
                                      stream if stream is not None else hip.stream_of(img.t)), "otp_h8_unpack")
    return out


def h16_weight_exponent(weight, scale=None) -> int:
    """Power of two k the fp16 engine stores a layer's (BatchNorm-folded) weights with: max |w * scale| * 2^k in [2^13, 2^14), so
    weights down to 2^-27 of the largest stay normal halves; the launch multiplies its fp32 sums by 2^-k (exact)."""
    w = weight.detach()
    m = w.abs().reshape(w.shape[0], -1).amax(dim=1)
    if scale is not None:
        m = m * scale.detach().abs().to(m.device, m.dtype)
    m = float(m.max())
    if not (m > 0.0 and math.isfinite(m)):
        return 0
    return max(-40, min(40, 14 - math.frexp(m)[1]))


def h16_conv_desc(x: H8, cout, stride, act=ACT_NONE, out: H8 = None, res: H8 = None, k=0):
    d = hip.H16ConvDesc()
    d.N, d.Cin, d.H, d.W, d.Cout, d.stride, d.act = x.N, x.C, x.H, x.W, cout, stride, act
    d.in_gtot, d.in_goff = x.gtot, x.goff
    d.out_gtot, d.out_goff = (out.gtot, out.goff) if out is not None else (0, 0)
    d.res_gtot, d.res_goff = (res.gtot, res.goff) if res is not None else (0, 0)
    d.out_scale = 2.0 ** -k
    return d


def h16_conv_supported(desc) -> bool:
    return bool(hip.lib().otp_h16_conv3x3_supported(desc))


def pack_h16_conv_weight(weight, scale=None, k=0):
    """(Cout, Cin, 3, 3) fp32 (x scale[cout] x 2^k) -> the half A-fragment image of csrc/h16.hip."""
    _require_gpu(weight)
    w = _f32(weight)
    cout, cin, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    L = hip.lib()
    packed = _image(L.otp_h16_conv3x3_weight_bytes(cout, cin), torch.int32, w.device,
                    RuntimeError, f"otp_h16_conv3x3: unsupported widths {cin} -> {cout}", zero=True)
    sc = _f32(scale, w.device)
    hip.check(L.otp_h16_conv3x3_pack_weight(hip.ptr(w), hip.ptr(sc), hip.ptr(packed), cout, cin, float(2.0 ** k), hip.stream_of(w)),
              "otp_h16_conv3x3_pack_weight")
    return packed


def h16_conv3x3_args(x: H8, wpacked, shift, out: H8, desc, res: H8 = None):
    return (_vp(x), hip.ptr(wpacked), hip.ptr(shift), _vp(res), _vp(out), desc)


def h16_conv3x3(x: H8, wpacked, shift, cout, stride=1, act=ACT_NONE, res: H8 = None, out: H8 = None, k=0, stream=None, desc=None):
    """out = act(conv3x3 pad 1 (x) + shift (+ res)) on H8 images (csrc/h16.hip)."""
    ho, wo = x.H // stride, x.W // stride
    out = h8_empty(x.N, cout, ho, wo, x.t.device) if out is None else out
    d = desc if desc is not None else h16_conv_desc(x, cout, stride, act, out, res, k)
    _launch(hip.lib().otp_h16_conv3x3, "otp_h16_conv3x3", h16_conv3x3_args(x, wpacked, shift, out, d, res), x.t, stream)
    return out


def h16_pointwise_supported(cin, cout) -> bool:
    return bool(hip.lib().otp_h16_pointwise_supported(int(cin), int(cout)))


def pack_h16_pointwise(weight, scale=None, shift=None, k=0):
    """(Cout, Cin[, 1, 1]) fp32 (x scale x 2^k) + shift -> the packed image of otp_h16_pointwise."""
    _require_gpu(weight)
    w = _f32(weight.reshape(weight.shape[0], -1))
    cout, cin = w.shape
    L = hip.lib()
    packed = _image(L.otp_h16_pointwise_weight_bytes(cin, cout), torch.int32, w.device,
                    RuntimeError, f"otp_h16_pointwise: unsupported widths {cin} -> {cout}", zero=True)
    sc, sh = _f32(scale, w.device), _f32(shift, w.device)
    hip.check(L.otp_h16_pointwise_pack(hip.ptr(w), hip.ptr(sc), hip.ptr(sh), hip.ptr(packed), cin, cout, float(2.0 ** k),
                                       hip.stream_of(w)), "otp_h16_pointwise_pack")
    return packed


def h16_pointwise_args(x: H8, packed, cout, out, relu=False, res: H8 = None, k=0):
    """``out``: an :class:`H8`, or a :class:`View` of an fp32 NCHW tensor."""
    return (_vp(x), hip.ptr(packed), _vp(res), _vp(out), int(isinstance(out, View)), x.N, x.C, cout, x.H * x.W, x.gtot, x.goff,
            *_slice(res), *_slice(out), int(relu), float(2.0 ** -k))


def h16_pointwise(x: H8, packed, cout, relu=False, res: H8 = None, out=None, k=0, stream=None):
    """out = act(W x + shift (+ res)): ``out`` an :class:`H8` (default: fresh) or a :class:`View` of an fp32 NCHW tensor."""
    if out is None:
        out = h8_empty(x.N, cout, x.H, x.W, x.t.device)
    _launch(hip.lib().otp_h16_pointwise, "otp_h16_pointwise", h16_pointwise_args(x, packed, cout, out, relu, res, k), x.t, stream)
    return out


def pack_h16_stem(weight, scale=None, shift=None):
    _require_gpu(weight)
    w = _f32(weight)
    cout = w.shape[0]
    L = hip.lib()
    packed = _image(L.otp_h16_stem_weight_bytes(cout), torch.int32, w.device,
                    RuntimeError, f"otp_h16_stem: unsupported width {cout}", zero=True)
    sc, sh = _f32(scale, w.device), _f32(shift, w.device)
    hip.check(L.otp_h16_stem_pack(hip.ptr(w), hip.ptr(sc), hip.ptr(sh), hip.ptr(packed), cout, hip.stream_of(w)), "otp_h16_stem_pack")
    return packed


def h16_stem(clip, packed, cout, frames, out: H8 = None, stream=None):
    """relu(conv3x3 s2 p1 of the frames of the fp32 clip (B, 3 F, H, W) + shift) as the H8 image of (F B, cout, Ho, Wo)."""
    _require_gpu(clip)
    b, c, h, w = clip.shape
    assert c == 3 * frames and clip.is_contiguous()
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = h8_empty(frames * b, cout, ho, wo, clip.device) if out is None else out
    _launch(hip.lib().otp_h16_stem, "otp_h16_stem", stem_conv_x3_args(clip, packed, out, frames, cout), clip, stream)
    return out


def h16_upsample_add_args(lows, factors, res: H8, out: H8, relu=True):
    """(arguments, ctypes arrays the caller keeps alive while the launch may still be issued) on dense H8 images."""
    lp = (ctypes.c_void_p * len(lows))(*[_vp(v) for v in lows])
    fp = (ctypes.c_int * len(lows))(*[int(f) for f in factors])
    return (lp, fp, len(lows), _vp(res), _vp(out), res.N, res.C, res.H, res.W, int(relu)), (lp, fp)


def h16_upsample_add(lows, factors, res: H8, relu=True, out: H8 = None, stream=None):
    """out = act(res + sum_k nearest_up(lows[k], factors[k])) on dense H8 images."""
    assert res.gtot * 8 == res.C and all(l.gtot * 8 == l.C for l in lows)
    out = h8_empty(res.N, res.C, res.H, res.W, res.t.device) if out is None else out
    args, _keep = h16_upsample_add_args(lows, factors, res, out, relu)
    _launch(hip.lib().otp_h16_upsample_add, "otp_h16_upsample_add", args, res.t, stream)
    return out


# ------------------------------------------------------------------------------------------------
# person detector (csrc/detect.hip; the reference's object_detector/YOLOv3)
# ------------------------------------------------------------------------------------------------
def letterbox(frames_u8, size, out=None):
    """uint8 RGB frames (B, H, W, 3) -> the detector's input (B, 3, size, size) float32 (``preprocess_img_for_yolo``,
    detector_utils.py:12-38): pad to a square with 127, area-average to ``size``, round to a uint8 level, / 255 - one kernel.
    Raises ``ValueError`` for ``max(H, W) < size``: there INTER_AREA is no area average any more."""
    _require_gpu(frames_u8)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise TypeError("frames_u8 must be a (B, H, W, 3) uint8 tensor")
    b, h, w, _ = frames_u8.shape
    size = int(size)
    if b < 1 or size < 1 or max(h, w) < size:
        raise ValueError(f"letterbox shrinks: a {h} x {w} frame cannot fill a {size} x {size} input")
    frames_u8 = frames_u8.contiguous()
    if out is None:
        out = torch.empty((b, 3, size, size), dtype=torch.float32, device=frames_u8.device)
    elif out.shape != (b, 3, size, size) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 (B, 3, size, size) tensor")
    _launch(hip.lib().otp_letterbox_u8, "otp_letterbox_u8", (hip.ptr(frames_u8), hip.ptr(out), b, h, w, size), frames_u8)
    return out


def leaky_pass_args(inp: View, out: View, shortcut: View = None, leaky=True, up=1):
    n, _, h, w = inp.t.shape
    assert out.C == inp.C and out.t.shape[0] == n and tuple(out.t.shape[2:]) == (h * up, w * up)
    assert shortcut is None or (shortcut.C == inp.C and shortcut.t.shape[0] == n and tuple(shortcut.t.shape[2:]) == (h, w))
    assert out.t.data_ptr() != inp.t.data_ptr()
    return (_vp(inp), _vp(shortcut), _vp(out), n, inp.C, h, w, int(leaky), int(up), inp.ctot, inp.coff, *_slice(shortcut),
            out.ctot, out.coff)


def leaky_pass(inp: View, out: View, shortcut: View = None, leaky=True, up=1, stream=None):
    """out = up( leaky_0.1(inp) + shortcut ) on channel-slice views: the pass behind a Darknet conv (``leaky``), fused with a
    following ``[shortcut]`` and / or nearest 2x ``[upsample]``; with ``leaky=False`` a plain add / upsample / slice copy."""
    _launch(hip.lib().otp_leaky_pass, "otp_leaky_pass", leaky_pass_args(inp, out, shortcut, leaky, up), inp.t, stream)
    return out


def yolo_decode_args(head, pred, anchors, num_classes, img_size, row_off):
    b, ch, g, g2 = head.shape
    a = len(anchors)
    assert g == g2 and ch == a * (5 + num_classes) and pred.shape[0] == b and pred.shape[2] == 5 + num_classes
    flat = (ctypes.c_double * (2 * a))(*[float(v) for wh in anchors for v in wh])
    return (hip.ptr(head), hip.ptr(pred), flat, b, a, num_classes, g, int(img_size), pred.shape[1], int(row_off)), flat


def yolo_decode(head, anchors, num_classes, img_size, pred=None, row_off=0):
    """Eval output of one ``[yolo]`` layer (models.py:123-165): ``head`` (B, A (5 + C), G, G) -> rows ``row_off ..`` of ``pred``
    (B, N, 5 + C) in the order (anchor, gy, gx), each ``(cx, cy, w, h, conf, cls...)`` in input pixels.  ``anchors``: A pairs
    (w, h) in input pixels.  A fresh (B, A G G, 5 + C) tensor when ``pred`` is None."""
    _require_gpu(head, pred)
    _check_f32(head, pred)
    if head.dim() != 4 or head.shape[2] != head.shape[3] or head.shape[1] != len(anchors) * (5 + num_classes):
        raise ValueError(f"head must be (B, {len(anchors)} * (5 + {num_classes}), G, G), got {tuple(head.shape)}")
    head = head.contiguous()
    rows = len(anchors) * head.shape[2] * head.shape[3]
    if pred is None:
        pred = torch.empty((head.shape[0], rows, 5 + num_classes), dtype=torch.float32, device=head.device)
    if (pred.dim() != 3 or pred.shape[0] != head.shape[0] or pred.shape[2] != 5 + num_classes or not pred.is_contiguous()
            or row_off < 0 or row_off + rows > pred.shape[1]):
        raise ValueError("pred must be a contiguous (B, N, 5 + C) tensor with room for the layer's rows at row_off")
    args, _keep = yolo_decode_args(head, pred, anchors, num_classes, img_size, row_off)
    _launch(hip.lib().otp_yolo_decode, "otp_yolo_decode", args, head)
    return pred


def frame_rescale(frame_hw, img_size):
    """``(pad_x // 2, pad_y // 2, unpad_w, unpad_h, w, h)`` of a frame, as detector_yolov3.py:79-83 evaluates them (Python
    floats); ``frame_hw=None`` gives the identity (boxes stay in input pixels)."""
    if frame_hw is None:
        return 0.0, 0.0, 1.0, 1.0, 1.0, 1.0
    h, w = int(frame_hw[0]), int(frame_hw[1])
    pad_x = max(h - w, 0) * (img_size / max(h, w))
    pad_y = max(w - h, 0) * (img_size / max(h, w))
    unpad_h = img_size - pad_y
    unpad_w = img_size - pad_x
    return float(pad_x // 2), float(pad_y // 2), float(unpad_w), float(unpad_h), float(w), float(h)


def box_nms_merge(pred, conf_thres=0.4, nms_thres=0.4, frame_hw=None, img_size=416, person_class=0, workspace=None):
    """Confidence filter, the reference's merging NMS (detector_utils.py:253-291) and its rescale to frame pixels
    (detector_yolov3.py:79-98) for every image of ``pred`` (B, N, 5 + C) float32 rows ``(cx, cy, w, h, conf, cls...)``; one
    launch, one workgroup per image, no limit on the number of candidates.  ``pred`` is not modified.  Returns device
    tensors ``(counts (B,) int32, dets (B, N, 6) float32, person_counts (B,) int32, person_boxes (B, N, 4) float64,
    person_scores (B, N) float32)``: ``dets`` rows ``(x1, y1, x2, y2, conf, class)`` in keep order, the ``person_*`` outputs the
    kept rows of ``person_class`` as ``x, y, w, h`` in pixels of a ``frame_hw`` = (H, W) frame.  Rows past a count are zero."""
    _require_gpu(pred)
    _check_f32(pred)
    if pred.dim() != 3 or pred.shape[2] < 6 or pred.shape[0] < 1 or pred.shape[1] < 1:
        raise ValueError(f"pred must be (B, N, 5 + C) with C >= 1, got {tuple(pred.shape)}")
    pred = pred.contiguous()
    b, n, k = pred.shape
    dev = pred.device
    need = hip.lib().otp_box_nms_merge_workspace(b, n)
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.int32, device=dev)
    counts = torch.empty(b, dtype=torch.int32, device=dev)
    dets = torch.empty((b, n, 6), dtype=torch.float32, device=dev)
    pcounts = torch.empty(b, dtype=torch.int32, device=dev)
    pboxes = torch.empty((b, n, 4), dtype=torch.float64, device=dev)
    pscores = torch.empty((b, n), dtype=torch.float32, device=dev)
    _launch(hip.lib().otp_box_nms_merge, "otp_box_nms_merge",
            (hip.ptr(pred), b, n, k - 5, float(conf_thres), float(nms_thres), int(person_class),
             *frame_rescale(frame_hw, img_size), n, hip.ptr(workspace), workspace.numel() * workspace.element_size(),
             hip.ptr(counts), hip.ptr(dets), hip.ptr(pcounts), hip.ptr(pboxes), hip.ptr(pscores)), pred)
    return counts, dets, pcounts, pboxes, pscores


# ------------------------------------------------------------------------------------------------
# temporal segment NMS (csrc/segnms.hip; the reference's thirdparty/utils nms_1d_cpu); the drop-in names are in segnms.py
# ------------------------------------------------------------------------------------------------
def _seg_batch(segs, scores, offsets):
    """Checked contiguous ``(segs (N, 2) f32, scores (N) f32, offsets (G+1) i32)`` of a segmented batch, N >= 1 and G >= 1."""
    _require_gpu(segs, scores, offsets)
    _check_f32(segs, scores)
    if segs.dim() != 2 or segs.shape[1] != 2 or scores.dim() != 1 or scores.shape[0] != segs.shape[0] or segs.shape[0] < 1:
        raise ValueError(f"segs must be (N, 2) and scores (N) with N >= 1, got {tuple(segs.shape)} and {tuple(scores.shape)}")
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.shape[0] < 2:
        raise ValueError("offsets must be a (G + 1) int32 tensor with G >= 1")
    return segs.contiguous(), scores.contiguous(), offsets.contiguous()


def _seg_workspace(g, n, device, workspace):
    need = hip.lib().otp_seg_nms_workspace(g, n)
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.int32, device=device)
    return workspace, workspace.numel() * workspace.element_size()


def seg_nms(segs, scores, offsets, iou_threshold, min_score=0.0, max_num=0, workspace=None):
    """Hard 1-D NMS (``nms_1d_cpu``, nms_cpu.cpp:19-58, behind ``NMSop``'s ``scores > min_score`` filter) of every group of a
    segmented batch in one launch: group g is rows ``offsets[g] .. offsets[g + 1]`` of ``segs`` (N, 2) / ``scores`` (N).
    Returns device tensors ``(counts (G,) int32, keep (N,) int32)``: rows ``offsets[g] ..`` of ``keep`` hold the group's kept
    indices (relative to its first row) in descending-score order, cut at ``max_num`` when it is > 0, then -1."""
    segs, scores, offsets = _seg_batch(segs, scores, offsets)
    g, n, dev = offsets.shape[0] - 1, segs.shape[0], segs.device
    workspace, nbytes = _seg_workspace(g, n, dev, workspace)
    counts = torch.empty(g, dtype=torch.int32, device=dev)
    keep = torch.empty(n, dtype=torch.int32, device=dev)
    _launch(hip.lib().otp_seg_nms, "otp_seg_nms",
            (hip.ptr(segs), hip.ptr(scores), hip.ptr(offsets), g, n, float(iou_threshold), float(min_score), int(max_num),
             hip.ptr(workspace), nbytes, hip.ptr(counts), hip.ptr(keep)), segs)
    return counts, keep


def seg_softnms(segs, scores, offsets, iou_threshold, sigma=0.5, min_score=0.0, method=2, max_num=0, workspace=None):
    """Soft 1-D NMS (``softnms_1d_cpu``, nms_cpu.cpp:67-160; ``method`` 0 hard, 1 linear, 2 gaussian) of every group of a
    segmented batch in one launch.  Returns device tensors ``(counts (G,) int32, dets (N, 3) float32, inds (N,) int32)``: rows
    ``offsets[g] + r`` hold the ``(x1, x2, decayed score)`` and the group-relative index of the segment taken in round r,
    cut at ``max_num`` when it is > 0; the group's remaining rows hold zeros and -1."""
    segs, scores, offsets = _seg_batch(segs, scores, offsets)
    if int(method) not in (0, 1, 2):
        raise ValueError(f"method must be 0 (hard), 1 (linear) or 2 (gaussian), got {method}")
    g, n, dev = offsets.shape[0] - 1, segs.shape[0], segs.device
    workspace, nbytes = _seg_workspace(g, n, dev, workspace)
    counts = torch.empty(g, dtype=torch.int32, device=dev)
    dets = torch.empty((n, 3), dtype=torch.float32, device=dev)
    inds = torch.empty(n, dtype=torch.int32, device=dev)
    _launch(hip.lib().otp_seg_softnms, "otp_seg_softnms",
            (hip.ptr(segs), hip.ptr(scores), hip.ptr(offsets), g, n, float(iou_threshold), float(sigma), float(min_score),
             int(method), int(max_num), hip.ptr(workspace), nbytes, hip.ptr(counts), hip.ptr(dets), hip.ptr(inds)), segs)
    return counts, dets, inds


def seg_voting_groups(nms_segs, nms_offsets, segs, scores, offsets, voting_thresh):
    """``seg_voting`` (nms.py:67-101) for the kept segments ``nms_segs`` (K, 2) of every group (``nms_offsets`` (G+1) int32)
    against all segments of the same group of the batch ``segs`` / ``scores`` / ``offsets``: (K, 2) score-weighted means of
    the segments with ``iou >= voting_thresh``; a row without such a segment is NaN, as in the reference."""
    segs, scores, offsets = _seg_batch(segs, scores, offsets)
    _require_gpu(nms_segs, nms_offsets)
    _check_f32(nms_segs)
    if nms_segs.dim() != 2 or nms_segs.shape[1] != 2:
        raise ValueError(f"nms_segs must be (K, 2), got {tuple(nms_segs.shape)}")
    if nms_offsets.dtype != torch.int32 or nms_offsets.shape != offsets.shape:
        raise ValueError("nms_offsets must be a (G + 1) int32 tensor like offsets")
    nms_segs, nms_offsets = nms_segs.contiguous(), nms_offsets.contiguous()
    k = nms_segs.shape[0]
    out = torch.empty((k, 2), dtype=torch.float32, device=segs.device)
    if k:
        _launch(hip.lib().otp_seg_voting, "otp_seg_voting",
                (hip.ptr(nms_segs), hip.ptr(nms_offsets), hip.ptr(segs), hip.ptr(scores), hip.ptr(offsets),
                 offsets.shape[0] - 1, k, segs.shape[0], float(voting_thresh), hip.ptr(out)), segs)
    return out


# ------------------------------------------------------------------------------------------------
# temporal detection AP (csrc/segap.hip; the reference's thirdparty/utils/metrics.py); the drop-in names are in segmetrics.py
# ------------------------------------------------------------------------------------------------
def _check_i32(what, t, min_len):
    if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < min_len:
        raise ValueError(f"{what} must be a 1-D int32 tensor of at least {min_len} entries")
    return t.contiguous()


def seg_ap_match(pred_seg, pred_offsets, gt_seg, gt_offsets, thresholds, workspace=None):
    """The greedy assignment of ``compute_average_precision_detection`` (metrics.py:243-271) for every (video, class) group
    and every tIoU threshold in one launch.  Group g is rows ``pred_offsets[g] .. pred_offsets[g + 1]`` of ``pred_seg`` (N, 2)
    float64, already in descending-score order inside the group, and rows ``gt_offsets[g] .. gt_offsets[g + 1]`` of ``gt_seg``
    (M, 2) float64.  ``thresholds``: up to ``OTP_SEG_AP_MAX_THRESHOLDS`` host floats.  Returns the device tensor ``match``
    (T, N) int32: the matched ground truth's row relative to the group's first, or -1 for a false positive."""
    _require_gpu(pred_seg, pred_offsets, gt_seg, gt_offsets)
    for what, t in (("pred_seg", pred_seg), ("gt_seg", gt_seg)):
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 2:
            raise ValueError(f"{what} must be an (n, 2) float64 tensor, got {tuple(t.shape)} {t.dtype}")
    pred_offsets, gt_offsets = _check_i32("pred_offsets", pred_offsets, 2), _check_i32("gt_offsets", gt_offsets, 2)
    if pred_offsets.shape != gt_offsets.shape:
        raise ValueError("pred_offsets and gt_offsets must describe the same G groups")
    thr = [float(v) for v in thresholds]
    t, n, m, g, dev = len(thr), pred_seg.shape[0], gt_seg.shape[0], pred_offsets.shape[0] - 1, pred_seg.device
    if not 1 <= t <= _K["OTP_SEG_AP_MAX_THRESHOLDS"]:
        raise ValueError(f"1 .. {_K['OTP_SEG_AP_MAX_THRESHOLDS']} thresholds, got {t}")
    if n == 0 or m == 0:                              # nothing to match: every prediction is a false positive
        return torch.full((t, n), -1, dtype=torch.int32, device=dev)
    need = hip.lib().otp_seg_ap_match_workspace(g, m, t)
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.int32, device=dev)
    match = torch.empty((t, n), dtype=torch.int32, device=dev)
    pred_seg, gt_seg = pred_seg.contiguous(), gt_seg.contiguous()
    _launch(hip.lib().otp_seg_ap_match, "otp_seg_ap_match",
            (hip.ptr(pred_seg), hip.ptr(pred_offsets), hip.ptr(gt_seg), hip.ptr(gt_offsets),
             (ctypes.c_double * t)(*thr), g, n, m, t, hip.ptr(workspace), workspace.numel() * workspace.element_size(),
             hip.ptr(match)), pred_seg)
    return match


def seg_ap(match, order, class_offsets, npos):
    """Interpolated AP (metrics.py:273-282, 312-321) of every (threshold, class) from ``match`` (T, N) int32 of
    :func:`seg_ap_match`.  ``order`` (N) int32: the rows of ``match`` in class-major order, descending score inside a class;
    ``class_offsets`` (C+1) int32 over ``order``; ``npos`` (C) int32: the ground truths of each class.  Returns ``ap`` (T, C)
    float64 on the device; a class without predictions gets 0."""
    _require_gpu(match, order, class_offsets, npos)
    if match.dtype != torch.int32 or match.dim() != 2:
        raise ValueError("match must be a (T, N) int32 tensor")
    t, n = match.shape
    order, class_offsets = _check_i32("order", order, 0), _check_i32("class_offsets", class_offsets, 2)
    c = class_offsets.shape[0] - 1
    npos = _check_i32("npos", npos, c)
    if order.shape[0] != n or npos.shape[0] != c or not 1 <= t <= _K["OTP_SEG_AP_MAX_THRESHOLDS"]:
        raise ValueError(f"order must have N = {n} entries, npos C = {c}, and T must be 1 .. {_K['OTP_SEG_AP_MAX_THRESHOLDS']}")
    if n == 0:
        return torch.zeros((t, c), dtype=torch.float64, device=match.device)
    ap = torch.empty((t, c), dtype=torch.float64, device=match.device)
    match = match.contiguous()
    _launch(hip.lib().otp_seg_ap, "otp_seg_ap",
            (hip.ptr(match), hip.ptr(order), hip.ptr(class_offsets), hip.ptr(npos), c, t, n, hip.ptr(ap)), match)
    return ap
