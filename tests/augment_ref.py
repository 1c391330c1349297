"""numpy restatement of the blurred crop of csrc/crop.hip (``otp_crop_clips_blur_u8``), in the kernel's float32 order.

``blur_frame``: torchvision 0.8 ``T.GaussianBlur((5, 9))`` of an (H, W, 3) uint8 frame as the kernel computes it: per
output byte acc = 0; for i in 0..8, for j in 0..4: acc = acc + w[i][j] * v (float32, every product and sum rounded),
v = the frame at column x + i - 4 (reflected at the left / right edges) and channel c + j - 2 (reflected across RGB);
then round half to even and clamp to [0, 255].
``blur_frame_conv``: the same blur as torchvision computes it (float32 ``conv2d`` with H groups): another summation order.
``crop_blur_ref``: the (B, F) crops of a pool with per-slot blur, flip and out-of-pool frames (tests/crop_ref.py).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests.crop_ref import warp_affine

RGB_REFLECT = [2, 1, 0, 1, 2, 1, 0]            # the RGB axis padded by 2 with reflection: [b, g, r, g, b, g, r]


def _reflect(idx, n):
    idx = np.where(idx < 0, -idx, idx)
    return np.where(idx > n - 1, 2 * (n - 1) - idx, idx)


def blur_frame(frame, table):
    """uint8 (H, W, 3), table (9, 5) float32 -> uint8 (H, W, 3) in the kernel's order."""
    x = np.asarray(frame).astype(np.float32)
    t = np.asarray(table, np.float32)
    W = x.shape[1]
    cols = _reflect(np.arange(-4, W + 4), W)
    acc = np.zeros(x.shape, np.float32)
    for i in range(9):
        xi = x[:, cols[i:i + W]]
        for j in range(5):
            acc = acc + t[i, j] * xi[:, :, RGB_REFLECT[j:j + 3]]
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def blur_frame_conv(frame, table):
    """torchvision 0.8 ``gaussian_blur`` of an (H, W, 3) uint8 tensor: reflect pad (2, 2, 4, 4), depthwise float32
    ``conv2d`` with H groups, ``round``."""
    x = torch.from_numpy(np.ascontiguousarray(frame)).unsqueeze(0).to(torch.float32)
    k = torch.from_numpy(np.asarray(table, np.float32)).expand(x.shape[1], 1, 9, 5)
    x = F.conv2d(F.pad(x, [2, 2, 4, 4], mode="reflect"), k, groups=x.shape[1])
    return torch.round(x.squeeze(0)).clamp(0, 255).to(torch.uint8).numpy()


def crop_blur_ref(pool, frame_idx, M, W, H, flip=None, blur=None, blur_on=None):
    """pool (S, Hp, Wp, 3) uint8, frame_idx (B, F), M (B, 2, 3), flip (B) or None, blur (B, F, 9, 5) or None, blur_on
    (B, F) or None (all on) -> (B, F, H, W, 3) uint8.  A flipped slot blurs the mirrored frame; an index outside [0, S)
    reads as an empty frame."""
    pool = np.asarray(pool)
    frame_idx = np.asarray(frame_idx)
    B, Fn = frame_idx.shape
    out = np.zeros((B, Fn, H, W, 3), np.uint8)
    blank = np.zeros(pool.shape[1:], np.uint8)
    for b in range(B):
        fl = bool(flip[b]) if flip is not None else False
        for f in range(Fn):
            k = int(frame_idx[b, f])
            src = pool[k] if 0 <= k < pool.shape[0] else blank
            if fl:
                src = src[:, ::-1]
            if blur is not None and (blur_on is None or blur_on[b][f]):
                src = blur_frame(src, blur[b][f])
            out[b, f] = warp_affine(src, M[b], W, H)
    return out
