"""Deformable position-sensitive RoI pooling: the autograd function and the three modules of the reference's
``thirdparty/deform_conv`` package (functions/deform_pool.py, modules/deform_pool.py) over the HIP operator of
``csrc/deform_pool.hip``.  Constructor arguments, sub-module names (``offset_fc``, ``mask_fc``: the ``state_dict`` keys) and
the zero-initialised last ``fc`` layers are the reference's; tensors are fp32 or fp64 and live on the GPU.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd import Function

from . import ops as deform_pool_cuda

__all__ = ["DeformRoIPoolingFunction", "deform_roi_pooling", "DeformRoIPooling", "DeformRoIPoolingPack",
           "ModulatedDeformRoIPoolingPack"]


class DeformRoIPoolingFunction(Function):
    """``deform_roi_pooling(data, rois, offset, spatial_scale, out_size, out_channels, no_trans, group_size=1,
    part_size=None, sample_per_part=4, trans_std=.0)`` (functions/deform_pool.py:7-66)."""

    @staticmethod
    def forward(ctx, data, rois, offset, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None,
                sample_per_part=4, trans_std=.0):
        ctx.geometry = (no_trans, spatial_scale, out_channels, group_size, out_size,
                        out_size if part_size is None else part_size, sample_per_part, trans_std)
        assert 0.0 <= trans_std <= 1.0
        if not data.is_cuda:
            raise NotImplementedError
        n = rois.shape[0]
        output = data.new_empty(n, out_channels, out_size, out_size)
        output_count = data.new_empty(n, out_channels, out_size, out_size)
        deform_pool_cuda.deform_psroi_pooling_cuda_forward(data, rois, offset, output, output_count, *ctx.geometry)
        if data.requires_grad or rois.requires_grad or offset.requires_grad:
            ctx.save_for_backward(data, rois, offset)
        ctx.output_count = output_count
        return output

    @staticmethod
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        data, rois, offset = ctx.saved_tensors
        grad_input = torch.zeros_like(data)
        grad_offset = torch.zeros_like(offset)
        deform_pool_cuda.deform_psroi_pooling_cuda_backward(grad_output.contiguous(), data, rois, offset, ctx.output_count,
                                                            grad_input, grad_offset, *ctx.geometry)
        return (grad_input, None, grad_offset) + (None,) * 8           # rois receive no gradient


deform_roi_pooling = DeformRoIPoolingFunction.apply


def _fc_stack(in_features, hidden, out_features, depth, gate=False):
    """``depth`` Linear layers with ReLU between them (a Sigmoid after the last with ``gate``); the last Linear starts at zero."""
    layers, width = [], in_features
    for i in range(depth):
        last = i == depth - 1
        layers.append(nn.Linear(width, out_features if last else hidden))
        width = hidden
        if not last:
            layers.append(nn.ReLU(inplace=True))
    nn.init.zeros_(layers[-1].weight)
    nn.init.zeros_(layers[-1].bias)
    if gate:
        layers.append(nn.Sigmoid())
    return nn.Sequential(*layers)


class DeformRoIPooling(nn.Module):

    def __init__(self, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None, sample_per_part=4,
                 trans_std=.0):
        super().__init__()
        self.spatial_scale = spatial_scale
        self.out_size = out_size
        self.out_channels = out_channels
        self.no_trans = no_trans
        self.group_size = group_size
        self.part_size = out_size if part_size is None else part_size
        self.sample_per_part = sample_per_part
        self.trans_std = trans_std

    def _pool(self, data, rois, offset, no_trans):
        if no_trans:
            offset = data.new_empty(0)
        return deform_roi_pooling(data, rois, offset, self.spatial_scale, self.out_size, self.out_channels, no_trans,
                                  self.group_size, self.part_size, self.sample_per_part, self.trans_std)

    def forward(self, data, rois, offset):
        return self._pool(data, rois, offset, self.no_trans)


def _offset_and_features(m, data, rois):
    """The offsets ``m.offset_fc`` predicts from the plain pooling of the RoIs, and that pooling flattened per RoI."""
    n = rois.shape[0]
    x = m._pool(data, rois, None, True).view(n, -1)
    return m.offset_fc(x).view(n, 2, m.out_size, m.out_size), x


class DeformRoIPoolingPack(DeformRoIPooling):
    """The pooling with its own offset branch: a plain pooling, ``offset_fc`` on it, then the deformable pooling."""

    def __init__(self, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None, sample_per_part=4,
                 trans_std=.0, num_offset_fcs=3, deform_fc_channels=1024):
        super().__init__(spatial_scale, out_size, out_channels, no_trans, group_size, part_size, sample_per_part, trans_std)
        self.num_offset_fcs = num_offset_fcs
        self.deform_fc_channels = deform_fc_channels
        if not no_trans:
            bins = self.out_size * self.out_size
            self.offset_fc = _fc_stack(bins * self.out_channels, deform_fc_channels, bins * 2, num_offset_fcs)

    def forward(self, data, rois):
        assert data.size(1) == self.out_channels
        if rois.shape[0] == 0:
            return data.new_empty(0, self.out_channels, self.out_size, self.out_size)
        if self.no_trans:
            return self._pool(data, rois, None, True)
        offset, _ = _offset_and_features(self, data, rois)
        return self._pool(data, rois, offset, False)


class ModulatedDeformRoIPoolingPack(DeformRoIPooling):
    """``DeformRoIPoolingPack`` times a per-bin gate ``mask_fc`` (sigmoid) computed from the same plain pooling."""

    def __init__(self, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None, sample_per_part=4,
                 trans_std=.0, num_offset_fcs=3, num_mask_fcs=2, deform_fc_channels=1024):
        super().__init__(spatial_scale, out_size, out_channels, no_trans, group_size, part_size, sample_per_part, trans_std)
        self.num_offset_fcs = num_offset_fcs
        self.num_mask_fcs = num_mask_fcs
        self.deform_fc_channels = deform_fc_channels
        if not no_trans:
            bins = self.out_size * self.out_size
            self.offset_fc = _fc_stack(bins * self.out_channels, deform_fc_channels, bins * 2, num_offset_fcs)
            self.mask_fc = _fc_stack(bins * self.out_channels, deform_fc_channels, bins, num_mask_fcs, gate=True)

    def forward(self, data, rois):
        assert data.size(1) == self.out_channels
        n = rois.shape[0]
        if n == 0:
            return data.new_empty(0, self.out_channels, self.out_size, self.out_size)
        if self.no_trans:
            return self._pool(data, rois, None, True)
        offset, x = _offset_and_features(self, data, rois)
        mask = self.mask_fc(x).view(n, 1, self.out_size, self.out_size)
        return self._pool(data, rois, offset, False) * mask
