"""Host side of the video -> crop step (reference dataset/PoseTrackDataset.py:228-420, utils/bbox.py, utils/transform.py).

Small per-person numpy arithmetic that decides *what* to crop: the 5-frame window, box -> center / scale, the affine crop
matrix and the Gaussian patch of the training targets.  The pixels themselves are cut on the GPU by
:func:`otpose_amd.ops.crop_clips` / :func:`otpose_amd.ops.pose_targets` (csrc/crop.hip).  Every function keeps the
reference's float32 / float64 steps, so its results equal the reference's bit for bit (tests/golden/crop.npz).
"""
from __future__ import annotations

import numpy as np

PIXEL_STD = 200.0


def box_to_center_scale(boxes_xywh, aspect_ratio, enlarge=1.0):
    """``xywh2cs`` (utils/bbox.py:7-36) over (N, 4) boxes ``x, y, w, h`` (top-left corner): returns ``center`` and
    ``scale`` (N, 2) float32, ``scale`` in units of 200 px, widened or heightened to ``aspect_ratio`` = width / height.
    Quirk kept: a box whose center x is exactly -1 is not enlarged."""
    b = np.asarray(boxes_xywh)
    b = b.astype(np.float32 if b.dtype == np.float32 else np.float64).reshape(-1, 4)
    x, y, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    center = np.stack([x + w * 0.5, y + h * 0.5], axis=1).astype(np.float32)
    ar = float(aspect_ratio)
    wide, tall = w > ar * h, w < ar * h
    h2 = np.where(wide, w * 1.0 / ar, h)
    w2 = np.where(tall, h * ar, w)
    scale = np.stack([w2 * 1.0 / PIXEL_STD, h2 * 1.0 / PIXEL_STD], axis=1).astype(np.float32)
    scale = np.where((center[:, 0] != -1)[:, None], scale * np.float32(enlarge), scale)
    return center, scale


def _affine_from_points(src, dst):
    """cv2.getAffineTransform's 6 x 6 system (three point pairs, float64) solved with LAPACK: (B, 3, 2) x 2 -> (B, 2, 3)."""
    src = src.astype(np.float64)
    dst = dst.astype(np.float64)
    n = src.shape[0]
    a = np.zeros((n, 6, 6))
    for i in range(3):
        a[:, 2 * i, 0:2] = src[:, i]
        a[:, 2 * i, 2] = 1.0
        a[:, 2 * i + 1, 3:5] = src[:, i]
        a[:, 2 * i + 1, 5] = 1.0
    rhs = dst.reshape(n, 6, 1)
    return np.linalg.solve(a, rhs).reshape(n, 2, 3)


def crop_matrix(center, scale, rot, output_size, inv=False):
    """``get_affine_transform`` (utils/transform.py:76-104, shift 0) for B persons: ``center`` / ``scale`` (B, 2) (taken
    as float32, as box_to_center_scale makes them), ``rot`` degrees (scalar or (B,)), ``output_size`` = (width, height).
    The three points are built in float32 like the reference; the 2 x 3 matrix is the float64 solve of the three point
    pairs.  Returns (B, 2, 3) float64: image -> crop, or crop -> image with ``inv``."""
    c = np.asarray(center, dtype=np.float32).reshape(-1, 2)
    s = np.asarray(scale, dtype=np.float32).reshape(-1, 2)
    n = c.shape[0]
    if s.shape[0] != n:
        raise ValueError("center and scale must both be (B, 2)")
    r = np.broadcast_to(np.asarray(rot, dtype=np.float64), (n,))
    dst_w, dst_h = output_size
    scale_tmp = s * np.float32(PIXEL_STD)
    rot_rad = np.pi * r / 180
    sn, cs = np.sin(rot_rad), np.cos(rot_rad)
    p1 = scale_tmp[:, 0].astype(np.float64) * -0.5                      # get_dir([0, src_w * -0.5], rot_rad)
    src_dir = np.stack([0.0 - p1 * sn, p1 * cs], axis=1)
    src = np.zeros((n, 3, 2), np.float32)
    dst = np.zeros((n, 3, 2), np.float32)
    src[:, 0] = c
    src[:, 1] = c.astype(np.float64) + src_dir
    dst_dir = np.array([0, dst_w * -0.5], np.float32)
    dst[:, 0] = [dst_w * 0.5, dst_h * 0.5]
    dst[:, 1] = np.array([dst_w * 0.5, dst_h * 0.5]) + dst_dir
    for p in (src, dst):                                                # get_3rd_point: b + (-d_y, d_x), d = a - b
        d = p[:, 0] - p[:, 1]
        p[:, 2] = p[:, 1] + np.stack([-d[:, 1], d[:, 0]], axis=1)
    return _affine_from_points(dst, src) if inv else _affine_from_points(src, dst)


def window(current_idx, num_frames, distance=2, posetrack18=True, available=None):
    """The spatio-temporal window of PoseTrackDataset._get_spatio_temporal_window (PoseTrackDataset.py:246-318).

    ``current_idx`` is the frame number as in the file name (PoseTrack18 numbers from 0, PoseTrack17 from 1),
    ``num_frames`` the length of the sequence.  Returns ``(frames, margin)``: the five frame numbers in the order
    cur, prev, next, pprev, nnext (the model's channel order) and ``margin = [left, right, lleft, rright]``.
    ``available`` (optional: a container of the frame numbers that exist, or a predicate) stands for the reference's
    file-existence test.

    The reference's quirks are kept:

    - ``nnext`` takes ``next_delta_range[0]``, so with two or more later frames it is the SAME frame as ``next``
      (``rright == right``), while ``pprev`` is two frames back;
    - PoseTrack17 numbering starts at 1, PoseTrack18 at 0 (the ranges are shifted accordingly);
    - with a single later frame ``next`` takes it and ``nnext`` falls back to the current frame (margin 0);
      likewise for the earlier side;
    - a ``prev`` / ``next`` frame that is not ``available`` falls back to the current one with margin 0;
      ``pprev`` / ``nnext`` are not checked (the reference only checks those two files).
    """
    cur, n = int(current_idx), int(num_frames)
    prev_r = list(range(1, min(cur + 1 if posetrack18 else cur, distance + 1)))
    next_r = list(range(1, min(n - cur if posetrack18 else n - cur + 1, distance + 1)))
    prev_d = prev_r[0] if prev_r else 0
    pprev_d = prev_r[1] if len(prev_r) > 1 else 0
    if not next_r:
        next_d = nnext_d = 0
    elif len(next_r) == 1:
        next_d, nnext_d = next_r[-1], 0
    else:
        next_d = nnext_d = next_r[0]
    left, lleft, right, rright = prev_d, pprev_d, next_d, nnext_d
    prev, nxt = cur - prev_d, cur + next_d
    if available is not None:
        has = available if callable(available) else (lambda k: k in available)
        if not has(prev):
            prev, left = cur, 0
        if not has(nxt):
            nxt, right = cur, 0
    return [cur, prev, nxt, cur - pprev_d, cur + nnext_d], [left, right, lleft, rright]


def gaussian_table(sigma):
    """The unnormalised (6 sigma + 1)^2 float32 Gaussian patch of generate_heatmaps (utils/heatmap.py:83-88), with its
    float32 arithmetic.  ``sigma`` must be a whole number (the patch bounds are integers)."""
    if float(sigma) != int(sigma) or int(sigma) < 1:
        raise ValueError(f"sigma must be a positive whole number, got {sigma!r}")
    sigma = int(sigma)
    size = 2 * sigma * 3 + 1
    x = np.arange(0, size, 1, np.float32)
    y = x[:, np.newaxis]
    x0 = y0 = size // 2
    return np.exp(- ((x - x0) ** 2 + (y - y0) ** 2) / (2 * sigma ** 2))
