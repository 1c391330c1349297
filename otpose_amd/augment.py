"""Training-time augmentation of the video -> crop step (reference dataset/PoseTrackDataset.py:343-388, utils/transform.py).

The random part of ``PoseTrackDataset._get_spatio_temporal_window`` in training mode: half-body crop, random scale and
rotation, horizontal flip and the per-frame Gaussian blur.  :func:`sample_augmentation` draws the same random numbers as
the reference, in the same order, sample after sample, so seeding ``np.random``, ``random`` and ``torch`` reproduces a
seeded reference run (tests/golden/augment.npz).  The deterministic part (crop matrix, window, Gaussian patch) stays in
:mod:`otpose_amd.crop`; the pixels are blurred and cut on the GPU by :func:`otpose_amd.ops.crop_clips` with ``blur=``.

numpy dtypes: the reference pins numpy 1.19, whose value-based casting keeps ``scale * np.clip(...)`` float32 and
evaluates the half-body sizes and the flipped ``center[0]`` in float64 before they are stored as float32.  numpy >= 2
(NEP 50) would make ``scale`` float64 and round the flipped center twice; this module spells out the 1.19 steps.
"""
from __future__ import annotations

import random
from dataclasses import dataclass

import numpy as np
import torch

PIXEL_STD = 200
FLIP_PAIRS = [[3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
UPPER_BODY_IDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)

BLUR_KERNEL = (5, 9)          # torchvision's (kx, ky): 5 taps along the RGB axis, 9 along the image width (see blur_table)
BLUR_SIGMA = (0.1, 5.0)
BLUR_PROB = 0.5
ROT_PROB = 0.6
FLIP_PROB = 0.5


def fliplr_joints(joints, vis, width, pairs=FLIP_PAIRS):
    """``fliplr_joints`` (utils/transform.py:59-73): x -> width - x - 1, left / right pairs swapped; returns
    ``(joints * vis, vis)`` as new float64 arrays, so the coordinates of invisible joints become 0."""
    j = np.array(joints, dtype=np.float64)
    v = np.array(vis, dtype=np.float64)
    j[:, 0] = width - j[:, 0] - 1
    for a, b in pairs:
        j[[a, b]] = j[[b, a]]
        v[[a, b]] = v[[b, a]]
    return j * v, v


def half_body(joints, vis, aspect_ratio, rng=np.random):
    """``half_body_transform`` (utils/transform.py:20-57): the box of the upper or the lower body's visible joints,
    widened to ``aspect_ratio`` and enlarged 1.5 times.  Returns ``(center, scale)`` (2,) float32.

    Quirks kept: the choice draws ``rng.randn() < 0.5`` (randn, not rand: the upper body is taken ~69 % of the time),
    always drawn even when the upper body is too small.  The reference's ``(None, None)`` return (fewer than 2 joints
    selected) cannot be reached behind the dataset's guard (more than NUM_JOINTS_HALF_BODY = 8 visible joints means at
    least 3 upper-body ones); it is returned here as well, and :func:`sample_augmentation` raises on it."""
    j = np.asarray(joints)
    v = np.asarray(vis)
    upper, lower = [], []
    for k in range(j.shape[0]):
        if v[k][0] > 0:
            (upper if k in UPPER_BODY_IDS else lower).append(j[k])
    if rng.randn() < 0.5 and len(upper) > 2:
        sel = upper
    else:
        sel = lower if len(lower) > 2 else upper
    if len(sel) < 2:
        return None, None
    sel = np.array(sel, dtype=np.float32)
    center = sel.mean(axis=0)[:2]
    lt, rb = np.amin(sel, axis=0), np.amax(sel, axis=0)
    w = np.float64(rb[0] - lt[0])                        # float32 difference, then numpy 1.19's float64 arithmetic
    h = np.float64(rb[1] - lt[1])
    ar = np.float64(aspect_ratio)
    if w > ar * h:
        h = w * 1.0 / ar
    elif w < ar * h:
        w = h * ar
    scale = np.array([w * 1.0 / PIXEL_STD, h * 1.0 / PIXEL_STD], dtype=np.float32)
    return center, scale * 1.5


def blur_table(sigma):
    """The (9, 5) float32 weights of torchvision 0.8 ``_get_gaussian_kernel2d((5, 9), [sigma, sigma])`` with its torch
    CPU operations: row i weighs the image column x + i - 4, column j the RGB channel c + j - 2 (reflected)."""
    s = float(sigma)

    def k1(n):
        half = (n - 1) * 0.5
        x = torch.linspace(-half, half, steps=n)
        pdf = torch.exp(-0.5 * (x / s).pow(2))
        return pdf / pdf.sum()

    kx, ky = k1(BLUR_KERNEL[0]), k1(BLUR_KERNEL[1])
    return torch.mm(ky[:, None], kx[None, :]).numpy()


@dataclass
class Augmentation:
    """One batch's augmentation: ``center`` / ``scale`` (B, 2) float32 after half-body, scale and flip; ``rotation``
    (B,) float64 degrees; ``flip`` (B,) bool; ``blur_sigma`` (B, F) float32, 0 = slot not blurred; ``joints`` /
    ``joints_vis`` (B, J, 3) float64, flipped (invisible joints zeroed when flipped)."""
    center: np.ndarray
    scale: np.ndarray
    rotation: np.ndarray
    flip: np.ndarray
    blur_sigma: np.ndarray
    joints: np.ndarray
    joints_vis: np.ndarray

    def blur_tables(self):
        """``(blur (B, F, 9, 5) float32, blur_on (B, F) uint8)`` for :func:`otpose_amd.ops.crop_clips`."""
        B, F = self.blur_sigma.shape
        tab = np.zeros((B, F, 9, 5), np.float32)
        on = (self.blur_sigma > 0).astype(np.uint8)
        for b, f in zip(*np.nonzero(on)):
            tab[b, f] = blur_table(self.blur_sigma[b, f])
        return tab, on


def sample_augmentation(joints, joints_vis, center, scale, width, *, scale_factor, rotation_factor, flip,
                        prob_half_body, num_joints_half_body, aspect_ratio=0.75, frames=5, np_rng=np.random,
                        py_rng=random, torch_gen=None):
    """The training branch of ``_get_spatio_temporal_window`` (PoseTrackDataset.py:343-388) for B samples.

    ``joints`` / ``joints_vis`` (B, J, 3) (the data items' ``joints_3d`` / ``joints_3d_vis``), ``center`` / ``scale``
    (B, 2) (box_to_center_scale), ``width`` the frame width (scalar or (B,)) that the flip mirrors over,
    ``aspect_ratio`` = IMAGE_SIZE width / height (0.75: 288 x 384).  Per sample, in the reference's order:

    1. ``np_rng.rand() < prob_half_body`` - drawn only when more than ``num_joints_half_body`` joints are visible - then
       the half-body ``np_rng.randn()`` (:func:`half_body`);
    2. ``scale *= clip(np_rng.randn() * sf + 1, 1 - sf, 1 + sf)`` (float32, as numpy 1.19 keeps it);
    3. ``py_rng.random() <= 0.6`` and only then the rotation ``np_rng.randn()``, clipped to +-2 rotation_factor;
    4. when ``flip``: ``py_rng.random() <= 0.5`` mirrors the joints (:func:`fliplr_joints`) and
       ``center[0] = width - center[0] - 1`` (evaluated in float64, stored float32: numpy 1.19);
    5. ``py_rng.random() <= 0.5`` blurs the sample: ``frames`` draws of ``torch.empty(1).uniform_(0.1, 5)``, slot
       order cur, prev, next, pprev, nnext (T.GaussianBlur.get_params).
    """
    jts = np.asarray(joints, dtype=np.float64)
    jvs = np.asarray(joints_vis, dtype=np.float64)
    if jts.ndim != 3 or jts.shape[-1] != 3 or jvs.shape != jts.shape:
        raise ValueError("joints and joints_vis must both be (B, J, 3)")
    B = jts.shape[0]
    cen = np.asarray(center, dtype=np.float32).reshape(B, 2)
    sca = np.asarray(scale, dtype=np.float32).reshape(B, 2)
    wid = np.broadcast_to(np.asarray(width), (B,))
    sf = scale_factor[0] if isinstance(scale_factor, (list, tuple)) else scale_factor
    rf = rotation_factor
    out_c, out_s = np.zeros((B, 2), np.float32), np.zeros((B, 2), np.float32)
    rot, fl = np.zeros(B, np.float64), np.zeros(B, bool)
    sig = np.zeros((B, frames), np.float32)
    out_j, out_v = jts.copy(), jvs.copy()
    for b in range(B):
        c, s = cen[b].copy(), sca[b].copy()
        j, v = jts[b].copy(), jvs[b].copy()
        if np.sum(v[:, 0]) > num_joints_half_body and np_rng.rand() < prob_half_body:
            c, s = half_body(j, v, aspect_ratio, np_rng)
            if c is None:
                raise ValueError(f"sample {b}: half_body found fewer than 2 joints")
        s = s * np.float32(np.clip(np_rng.randn() * sf + 1, 1 - sf, 1 + sf))
        r = float(np.clip(np_rng.randn() * rf, -rf * 2, rf * 2)) if py_rng.random() <= ROT_PROB else 0.0
        if flip and py_rng.random() <= FLIP_PROB:
            j, v = fliplr_joints(j, v, int(wid[b]), FLIP_PAIRS)
            c[0] = np.float64(int(wid[b])) - np.float64(c[0]) - 1
            fl[b] = True
        if py_rng.random() <= BLUR_PROB:
            for f in range(frames):
                sig[b, f] = torch.empty(1).uniform_(BLUR_SIGMA[0], BLUR_SIGMA[1], generator=torch_gen).item()
        out_c[b], out_s[b], rot[b] = c, s, r
        out_j[b], out_v[b] = j, v
    return Augmentation(out_c, out_s, rot, fl, sig, out_j, out_v)
