"""Deformable PS-RoI pooling (csrc/deform_pool.hip): the pybind entry points of the reference's second native module
(deform_pool_cuda)."""
from __future__ import annotations

import torch

from .. import hip
from .base import _K, require_gpu

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
    require_gpu(input, bbox, trans, out, top_count)
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
    require_gpu(out_grad, input, bbox, trans, top_count, input_grad, trans_grad)
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
