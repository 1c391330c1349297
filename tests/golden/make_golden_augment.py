#!/usr/bin/env python
"""Generate tests/golden/augment.npz by RUNNING the reference's training-mode ``_get_spatio_temporal_window``
(dataset/PoseTrackDataset.py:228-447) on seeded frames (build container only).

Run from the repo root:  ``python tests/golden/make_golden_augment.py``

The reference is imported with the stubs of make_golden.py.  The dataset object is made with ``object.__new__`` and the
attributes ``BaseDataset`` / ``__init__`` set (PoseTrack18 training config, ``transform = None``: the recorded crops are
the uint8 warps).  Stubs on top:

- ``cv2.imread`` returns the seeded frame of the path's number in BGR, ``cv2.cvtColor`` reverses the channels and marks
  the frame so that ``frame.shape`` yields numpy integers (see ``_Frame``), ``cv2.warpAffine`` is tests/crop_ref's
  ``warp_affine``, ``cv2.getAffineTransform`` the float64 three-point solve of make_golden_crop.py;
- ``torchvision.transforms.GaussianBlur`` restates torchvision 0.8 (``get_params`` draws ``uniform_(0.1, 5)``;
  ``gaussian_blur`` on an (H, W, 3) uint8 tensor = a depthwise float32 ``conv2d`` with H groups: 9 taps along the image
  width, 5 along the RGB axis, reflect padding, ``round``) and records every sigma;
- ``pycocotools`` / ``motmetrics`` / ``shapely`` / ``yacs`` are empty modules when they are missing;
- empty frame files in a temporary directory let ``osp.exists`` see the window.

numpy 1.19 dtypes: the module runs with an ``np`` whose ``clip`` returns a Python float (numpy >= 2 would make ``scale``
float64), and ``_Frame.shape`` gives numpy integers so that ``width - center[0] - 1`` is evaluated in float64 as under
1.19's value-based casting.  ``np.random``, ``random`` and ``torch`` are seeded once; the samples run in order.
"""
from __future__ import annotations

import copy
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference, save     # noqa: E402
from make_golden_crop import _three_point_solve     # noqa: E402
from tests.crop_ref import warp_affine              # noqa: E402

S, HF, WF = 6, 60, 80                 # frames, frame height, frame width
IMAGE_SIZE = [32, 64]                 # crop (W, H)
HEATMAP_SIZE = [8, 16]
SIGMA = 2
J = 17
SEED = 3


class _Frame(np.ndarray):
    """A decoded frame whose ``shape`` holds numpy integers: numpy 1.19 promoted ``shape[1] - float32`` to float64."""

    @property
    def shape(self):
        return tuple(np.int64(d) for d in np.asarray(self).shape)


class _NP119:
    """The dataset module's ``np``: numpy, except that ``clip`` of a scalar returns a Python float (the float32
    ``scale * clip(...)`` of numpy 1.19)."""

    def __getattr__(self, k):
        return getattr(np, k)

    @staticmethod
    def clip(*a, **k):
        r = np.clip(*a, **k)
        return float(r) if np.ndim(r) == 0 else r


class _GaussianBlur:
    """torchvision 0.8 ``T.GaussianBlur`` on a tensor (transforms.py / functional_tensor.py), sigmas recorded."""
    sigmas = []

    def __init__(self, kernel_size, sigma):
        self.kernel_size, self.sigma = kernel_size, sigma

    @staticmethod
    def _k1(n, s):
        half = (n - 1) * 0.5
        x = torch.linspace(-half, half, steps=n)
        pdf = torch.exp(-0.5 * (x / s).pow(2))
        return pdf / pdf.sum()

    def __call__(self, img):
        s = torch.empty(1).uniform_(self.sigma[0], self.sigma[1]).item()
        _GaussianBlur.sigmas.append(s)
        kx, ky = self._k1(self.kernel_size[0], s), self._k1(self.kernel_size[1], s)
        k = torch.mm(ky[:, None], kx[None, :])
        k = k.expand(img.shape[-3], 1, k.shape[0], k.shape[1])
        x = img.unsqueeze(0).to(torch.float32)
        p = [self.kernel_size[0] // 2, self.kernel_size[0] // 2, self.kernel_size[1] // 2, self.kernel_size[1] // 2]
        x = F.pad(x, p, mode="reflect")
        x = F.conv2d(x, k, groups=x.shape[-3])
        return torch.round(x.squeeze(0)).to(img.dtype)


def _frames():
    """Seeded RGB frames: 5 x 5 blocks of random colours (sharp edges for the blur, compressible) + a few stripes."""
    rng = np.random.RandomState(11)
    out = np.zeros((S, HF, WF, 3), np.uint8)
    for k in range(S):
        blocks = rng.randint(0, 256, (HF // 5, WF // 5, 3)).astype(np.uint8)
        f = np.kron(blocks, np.ones((5, 5, 1), np.uint8))
        f[:, rng.randint(0, WF, 6)] = rng.randint(0, 256, 3).astype(np.uint8)
        f[:, :2] = rng.randint(0, 256, (HF, 2, 3))             # columns where the edge reflection applies
        f[:, -2:] = rng.randint(0, 256, (HF, 2, 3))
        out[k] = f
    return out


def _items(ref_box2cs, aspect, img_dir):
    """24 data items of one 6-frame PoseTrack18 sequence: windows at both ends, all / most / few joints visible,
    invisible joints with coordinates, joints at the box edges."""
    rng = np.random.RandomState(5)
    items = []
    for n in range(24):
        cur = [0, 5, 2, 3, 1, 4][n % 6]
        x, y = rng.uniform(-5, 50), rng.uniform(-5, 25)
        w, h = rng.uniform(12, 40), rng.uniform(20, 45)
        jt = np.zeros((J, 3))
        jt[:, 0] = rng.uniform(x, x + w, J)
        jt[:, 1] = rng.uniform(y, y + h, J)
        jt[:4, :2] = [[x, y], [x + w, y + h], [x, y + h], [x + w, y]]              # box corners: crop edges
        jt[:, :2] = np.round(jt[:, :2] * 4) / 4
        vis = np.ones((J, 3))
        vis[:, 2] = 0
        kind = n % 4
        if kind == 1:
            vis[rng.choice(J, 4, replace=False), :2] = 0        # 13 visible: half-body eligible
        elif kind == 2:
            vis[11:, :2] = 0                                     # no lower body: upper forced
            vis[rng.choice(11, 1), :2] = 0
        elif kind == 3:
            vis[rng.choice(J, 10, replace=False), :2] = 0       # 7 visible: no half-body draw
        box = [max(0.0, x), max(0.0, y), w, h]
        c, s = ref_box2cs(box, aspect, 1.25)
        items.append({"image": os.path.join(img_dir, "%06d.jpg" % cur), "center": c, "scale": s, "box": box,
                      "joints_3d": jt, "joints_3d_vis": vis, "filename": "", "imgnum": 0, "nframes": S,
                      "frame_id": cur})
    return items


def main():
    for name in ("pycocotools", "pycocotools.coco", "motmetrics", "shapely", "shapely.geometry", "yacs",
                 "yacs.config"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["pycocotools.coco"].COCO = getattr(sys.modules["pycocotools.coco"], "COCO", object)
    sys.modules["shapely"].geometry = sys.modules["shapely.geometry"]
    sys.modules["yacs.config"].CfgNode = getattr(sys.modules["yacs.config"], "CfgNode", dict)
    import_reference()
    frames = _frames()
    cv2 = sys.modules["cv2"]
    cv2.COLOR_BGR2RGB, cv2.INTER_LINEAR = 4, 1
    cv2.imread = lambda path: np.ascontiguousarray(frames[int(os.path.basename(path)[:-4])][..., ::-1])
    cv2.cvtColor = lambda img, code: np.ascontiguousarray(img[..., ::-1]).view(_Frame)
    cv2.warpAffine = lambda src, M, dsize, flags=None: warp_affine(np.asarray(src), M, int(dsize[0]), int(dsize[1]))
    cv2.getAffineTransform = _three_point_solve
    sys.modules["torchvision.transforms"].GaussianBlur = _GaussianBlur
    import dataset.PoseTrackDataset as P
    import utils.bbox as BB
    P.np = _NP119()
    T = sys.modules["torchvision.transforms"]
    P.T = T

    reads, flips = [], []
    imread = cv2.imread
    cv2.imread = lambda path: (reads.append(int(os.path.basename(path)[:-4])), imread(path))[1]
    fliplr = P.fliplr_joints

    def fliplr_rec(joints, vis, width, pairs):
        j, v = fliplr(joints, vis, width, pairs)
        flips.append((j.copy(), v.copy()))
        return j, v

    P.fliplr_joints = fliplr_rec

    ds = object.__new__(P.PoseTrackDataset)
    image_size = np.array(IMAGE_SIZE)
    ds.__dict__.update(
        phase="train", train=True, is_posetrack18=True, pixel_std=200, image_size=image_size,
        image_width=image_size[0], image_height=image_size[1], aspect_ratio=image_size[0] * 1.0 / image_size[1],
        heatmap_size=np.array(HEATMAP_SIZE), scale_factor=[0.35, 0.35], rotation_factor=45, flip=True,
        color_rgb=True, num_joints_half_body=8, prob_half_body=0.3, num_joints=J, use_different_joints_weight=False,
        flip_pairs=[[3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]],
        joints_weight=np.array([1., 1., 1., 1., 1., 1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5],
                               dtype=np.float32).reshape((J, 1)),
        upper_body_ids=(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10), lower_body_ids=(11, 12, 13, 14, 15, 16),
        transform=None, distance=2, sigma=SIGMA, model_input_type="spatiotemporal_window")

    with tempfile.TemporaryDirectory() as tmp:
        for k in range(S):
            open(os.path.join(tmp, "%06d.jpg" % k), "wb").close()
        items = _items(BB.box2cs, ds.aspect_ratio, tmp)
        np.random.seed(SEED)
        random.seed(SEED)
        torch.manual_seed(SEED)
        rec = {k: [] for k in ("frame_idx", "margin", "center", "scale", "rotation", "flip", "sigma", "crops",
                               "target", "target_weight", "joints", "joints_vis")}
        for it in items:
            reads.clear()
            n_flip, n_sig = len(flips), len(_GaussianBlur.sigmas)
            out = ds._get_spatio_temporal_window(copy.deepcopy(it))
            meta = out[7]
            rec["frame_idx"].append(reads[:5])
            rec["margin"].append([meta["margin_left"], meta["margin_right"], meta["margin_lleft"],
                                  meta["margin_rright"]])
            rec["crops"].append(np.stack([np.asarray(o) for o in out[:5]]))
            rec["target"].append(out[5].numpy())
            rec["target_weight"].append(out[6].numpy())
            rec["center"].append(np.asarray(meta["center"]))
            rec["scale"].append(np.asarray(meta["scale"]))
            rec["rotation"].append(float(meta["rotation"]))
            fl = len(flips) > n_flip
            rec["flip"].append(fl)
            rec["joints"].append(flips[-1][0] if fl else it["joints_3d"])
            rec["joints_vis"].append(flips[-1][1] if fl else it["joints_3d_vis"])
            sig = _GaussianBlur.sigmas[n_sig:]
            rec["sigma"].append(sig if sig else [0.0] * 5)

    g = {k: np.asarray(v) for k, v in rec.items()}
    for k in ("center", "scale", "sigma", "target", "target_weight"):
        assert g[k].dtype == np.float32 or k == "sigma", (k, g[k].dtype)
    g["sigma"] = g["sigma"].astype(np.float32)
    blurred, rot = g["sigma"][:, 0] > 0, g["rotation"] != 0
    for name, mask in (("flip", g["flip"]), ("blur", blurred), ("rotation", rot)):
        assert mask.any() and not mask.all(), f"seed {SEED}: {name} does not take both branches"
    assert g["frame_idx"].min() == 0 and g["frame_idx"].max() == S - 1
    save("augment", frames=frames, item_center=np.stack([it["center"] for it in items]),
         item_scale=np.stack([it["scale"] for it in items]), item_joints=np.stack([it["joints_3d"] for it in items]),
         item_joints_vis=np.stack([it["joints_3d_vis"] for it in items]),
         item_frame=np.array([it["frame_id"] for it in items]), seed=np.array([SEED]), image_size=image_size,
         heatmap_size=np.array(HEATMAP_SIZE), sigma_heatmap=np.array([SIGMA]), **g)


if __name__ == "__main__":
    main()
