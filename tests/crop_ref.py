"""numpy restatement of csrc/crop.hip (integer arithmetic in int64, doubles as numpy float64 element-wise operations).

``warp_affine``: cv2.warpAffine(src, M, (W, H), INTER_LINEAR, BORDER_CONSTANT 0) of OpenCV <= 4.10 for uint8 RGB frames
(WarpAffineInvoker's 1/1024 px row origin + column delta, remapBilinear's 1/32 px fixed-point weights).
``crop_ref``: the crops of a (B, F) window from a frame pool, as the kernel reads them (flip, out-of-range frames).
``pose_targets_ref``: joint transform + visibility cut + generate_heatmaps.
"""
from __future__ import annotations

import numpy as np

AB = 1024
ROUND_DELTA = 16


def invert(M):
    """warpAffine's inversion of a forward 2 x 3 matrix (double, every operation rounded)."""
    M = np.asarray(M, np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A0, A1, A3, A4 = M[1, 1] * D, M[0, 1] * -D, M[1, 0] * -D, M[0, 0] * D
    A2 = -A0 * M[0, 2] - A1 * M[1, 2]
    A5 = -A3 * M[0, 2] - A4 * M[1, 2]
    return A0, A1, A2, A3, A4, A5


def _sat_rint(v):
    r = np.rint(v)
    out = np.where(np.isnan(r), -2 ** 31, np.clip(np.nan_to_num(r), -2 ** 31, 2 ** 31 - 1))
    return out.astype(np.int64)


def _wrap32(v):
    return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31


def source_coords(M, W, H):
    """(sx, sy, ax, ay) int64 (H, W): the integer source corner and the 1/32 px fractions of every output pixel."""
    A0, A1, A2, A3, A4, A5 = invert(M)
    y = np.arange(H, dtype=np.float64)[:, None]
    x = np.arange(W, dtype=np.float64)[None, :]
    X0 = _wrap32(_sat_rint((A1 * y + A2) * AB) + ROUND_DELTA)
    Y0 = _wrap32(_sat_rint((A4 * y + A5) * AB) + ROUND_DELTA)
    X = _wrap32(X0 + _sat_rint(A0 * x * AB)) >> 5
    Y = _wrap32(Y0 + _sat_rint(A3 * x * AB)) >> 5
    sx = np.clip(X >> 5, -32768, 32767)
    sy = np.clip(Y >> 5, -32768, 32767)
    return sx, sy, X & 31, Y & 31


def warp_affine(src, M, W, H, flip=False):
    """uint8 (Hs, Ws, 3) -> uint8 (H, W, 3); ``flip`` warps src[:, ::-1] (read as mirrored columns)."""
    src = np.asarray(src)
    Hs, Ws = src.shape[:2]
    sx, sy, ax, ay = source_coords(M, W, H)
    acc = np.zeros((H, W, 3), np.int64)
    for dy, dx, wgt in ((0, 0, (32 - ax) * (32 - ay) * 32), (0, 1, ax * (32 - ay) * 32),
                        (1, 0, (32 - ax) * ay * 32), (1, 1, ax * ay * 32)):
        c, r = sx + dx, sy + dy
        if flip:
            c = Ws - 1 - c
        ok = (c >= 0) & (c < Ws) & (r >= 0) & (r < Hs)
        v = src[np.where(ok, r, 0), np.where(ok, c, 0)].astype(np.int64) * ok[..., None]
        acc += v * wgt[..., None]
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def crop_ref(pool, frame_idx, M, W, H, flip=None):
    """pool (S, Hp, Wp, 3) uint8, frame_idx (B, F), M (B, 2, 3), flip (B) or None -> (B, F, H, W, 3) uint8 crops."""
    pool = np.asarray(pool)
    frame_idx = np.asarray(frame_idx)
    B, F = frame_idx.shape
    out = np.zeros((B, F, H, W, 3), np.uint8)
    blank = np.zeros(pool.shape[1:], np.uint8)
    for b in range(B):
        fl = bool(flip[b]) if flip is not None else False
        for f in range(F):
            k = int(frame_idx[b, f])
            out[b, f] = warp_affine(pool[k] if 0 <= k < pool.shape[0] else blank, M[b], W, H, fl)
    return out


def affine_points(M, pts):
    """exec_affine_transform with the plain left-to-right sums (the kernel's order): (B, 2, 3) x (B, J, 2) -> (B, J, 2)."""
    M = np.asarray(M, np.float64)
    x, y = pts[..., 0], pts[..., 1]
    return np.stack([M[:, None, 0, 0] * x + M[:, None, 0, 1] * y + M[:, None, 0, 2],
                     M[:, None, 1, 0] * x + M[:, None, 1, 1] * y + M[:, None, 1, 2]], axis=-1)


def visibility_cut(pts, vis, W, H):
    """PoseTrackDataset.py:408-414: a joint outside [0, W] x [0, H] becomes invisible."""
    x, y = pts[..., 0], pts[..., 1]
    return np.where((x < 0) | (y < 0) | (x > W) | (y > H), np.float32(0), vis).astype(np.float32)


def pose_targets_ref(joints, vis, M, sigma, image_size, heatmap_size):
    """joints (B, J, 2) float64, vis (B, J) float32, M (B, 2, 3) -> target (B, J, h, w), target_weight (B, J, 1)."""
    from otpose_amd.crop import gaussian_table
    W, H = image_size
    w, h = heatmap_size
    joints = np.asarray(joints, np.float64)[..., :2]
    vis = np.asarray(vis, np.float32)
    pts = np.where((vis > 0)[..., None], affine_points(M, joints), joints)
    v = visibility_cut(pts, vis, W, H)
    g = gaussian_table(sigma)
    t3 = 3 * int(sigma)
    B, J = vis.shape
    target = np.zeros((B, J, h, w), np.float32)
    weight = v.reshape(B, J, 1).copy()
    for b in range(B):
        for j in range(J):
            mx = int(pts[b, j, 0] / (W / w) + 0.5)
            my = int(pts[b, j, 1] / (H / h) + 0.5)
            ul, br = (mx - t3, my - t3), (mx + t3 + 1, my + t3 + 1)
            if ul[0] >= w or ul[1] >= h or br[0] < 0 or br[1] < 0:
                weight[b, j, 0] = 0
                continue
            if weight[b, j, 0] > 0.5:
                x0, x1, y0, y1 = max(0, ul[0]), min(br[0], w), max(0, ul[1]), min(br[1], h)
                target[b, j, y0:y1, x0:x1] = g[y0 - ul[1]:y1 - ul[1], x0 - ul[0]:x1 - ul[0]]
    return target, weight
