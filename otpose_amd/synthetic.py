"""Seeded synthetic weights and inputs for parity tests and ``bench.py``.

There is no network for datasets or checkpoints, and the reference's default initialisation
(conv N(0, 1e-3), model/OTPose.py:439-443; residual scale 1e-4, model/blocks.py:289) produces
heatmaps of magnitude 1e-19, which would make a 1e-3 max-abs check
vacuous.  :func:`fill_synthetic_` therefore writes a *calibrated* recipe into any module (or
state dict) that has the reference key set: fan-in scaled convolutions, damped residual branches,
randomised BatchNorm running statistics, residual scales of 0.5, and output layers scaled so
that every compared heatmap is O(0.1 - 1), offsets have a spread of a few pixels (samples cross
the image border) and DCN masks are O(1).

Everything is drawn from one CPU ``torch.Generator`` in a fixed (sorted-by-name) order so that
every process - the reference import that produced tests/golden, the oracle, and the HIP path on
any number of GPUs - sees identical tensors.  Nothing here depends on ``oracle/``.
"""
from __future__ import annotations

import math
import re
from typing import Dict, Tuple

import torch

WEIGHT_SEED = 1234
INPUT_SEED = 4321

# output-layer gains found by measuring activation spreads of the recipe on the oracle
# (tests/golden/make_golden.py --calibrate prints them); keyed by HRNet width and image size.
_GAINS = {
    "default": {"hrnet_final": 0.02, "final12": 0.15, "offset": 0.1, "mask": 0.02},
    "w8_64x96": {"hrnet_final": 0.0412139, "final12": 0.143413, "offset": 0.110823, "mask": 0.017563},
    "w32_192x256": {"hrnet_final": 0.0148956, "final12": 0.0547529, "offset": 0.0583049, "mask": 0.00918305},
    "w48_288x384": {"hrnet_final": 0.0220267, "final12": 0.19774, "offset": 0.131595, "mask": 0.0207387},
}


def gains_for(cfg) -> Dict[str, float]:
    """Calibrated output-layer gains of a built-in configuration (``default`` when unknown)."""
    w, h = cfg["MODEL"]["IMAGE_SIZE"]
    width = cfg["MODEL"]["EXTRA"]["STAGE2"]["NUM_CHANNELS"][0]
    return dict(_GAINS.get(f"w{width}_{w}x{h}", _GAINS["default"]))


def _fan_in(shape) -> int:
    n = 1
    for s in shape[1:]:
        n *= s
    return max(n, 1)


def _normal(gen, shape, std):
    return torch.randn(shape, generator=gen, dtype=torch.float32) * std


def synthetic_state_dict(shapes: Dict[str, Tuple[int, ...]], seed: int = WEIGHT_SEED,
                         gains: Dict[str, float] | None = None) -> Dict[str, torch.Tensor]:
    """Generate a tensor for every (name, shape) of an OTPose state dict; ``pos_embd`` buffers and
    ``num_batches_tracked`` counters are left out (their constructor values are kept)."""
    g = dict(_GAINS["default"])
    g.update(gains or {})
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    out: Dict[str, torch.Tensor] = {}
    for name in sorted(shapes):
        shape = tuple(shapes[name])
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked" or leaf == "pos_embd":
            continue
        is_bn_like = len(shape) == 1 and leaf in ("weight", "bias", "running_mean", "running_var")
        # ---- BatchNorm (eval mode uses the running statistics) --------------------------------
        if leaf == "running_mean":
            out[name] = _normal(gen, shape, 0.1)
        elif leaf == "running_var":
            out[name] = 0.8 + 0.4 * torch.rand(shape, generator=gen)
        elif is_bn_like and leaf == "weight" and _is_bn(name, shapes):
            gamma = 1.0 + _normal(gen, shape, 0.1)
            out[name] = gamma * _bn_branch_gain(name)
        elif is_bn_like and leaf == "bias" and _is_bn(name, shapes):
            out[name] = _normal(gen, shape, 0.1)
        # ---- transformer pieces ---------------------------------------------------------------
        elif leaf == "scale":                       # AffineDropPath
            out[name] = 0.5 + _normal(gen, shape, 0.05)
        elif len(shape) == 3 and shape[0] == 1 and leaf == "weight":   # channel LayerNorm gamma
            out[name] = 1.0 + _normal(gen, shape, 0.1)
        elif len(shape) == 3 and shape[0] == 1 and leaf == "bias":     # channel LayerNorm beta
            out[name] = _normal(gen, shape, 0.1)
        elif len(shape) == 3 and leaf == "weight":  # Conv1d (depthwise k3 or pointwise)
            out[name] = _normal(gen, shape, 1.0 / math.sqrt(_fan_in(shape)))
        # ---- DCN ------------------------------------------------------------------------------
        elif ".deform_conv." in name and leaf == "weight":
            w = _normal(gen, shape, 0.5 / math.sqrt(_fan_in(shape)))
            k = shape[2] // 2
            for o in range(min(shape[0], shape[1])):
                w[o, o, k, k] += 1.0                # identity at the centre tap + noise
            out[name] = w
        elif name.startswith("offsets_list"):
            out[name] = _normal(gen, shape, g["offset"] / math.sqrt(_fan_in(shape)))
        elif name.startswith("masks_list"):
            out[name] = _normal(gen, shape, g["mask"] / math.sqrt(_fan_in(shape)))
        # ---- output 1x1 layers ----------------------------------------------------------------
        elif name == "rough_pose_estimation_net.final_layer.weight":
            out[name] = _normal(gen, shape, g["hrnet_final"] / math.sqrt(_fan_in(shape)))
        elif re.match(r"final_layer[12]\.weight", name):
            out[name] = _normal(gen, shape, g["final12"] / math.sqrt(_fan_in(shape)))
        # ---- generic conv weights / biases ----------------------------------------------------
        elif leaf == "weight" and len(shape) == 4:
            out[name] = _normal(gen, shape, math.sqrt(2.0 / _fan_in(shape)))
        elif leaf == "bias":
            out[name] = _normal(gen, shape, 0.05)
        else:
            raise KeyError(f"synthetic recipe has no rule for {name} {shape}")
    return out


def _is_bn(name: str, shapes) -> bool:
    stem = name.rsplit(".", 1)[0]
    return (stem + ".running_var") in shapes


def _bn_branch_gain(name: str) -> float:
    """Damp the last BN of every residual branch so depth does not blow activations up."""
    if re.search(r"\.bn2\.weight$", name) and re.search(r"(branches|layer1)\.", name) and ".bn3" not in name:
        # BasicBlock.bn2 closes the residual branch; Bottleneck.bn2 does not (bn3 does)
        return 0.25 if "layer1" not in name else 1.0
    if name.endswith(".bn3.weight"):
        return 0.25
    if ".fuse_layers." in name:
        return 0.3
    if ".conv_bn_relu3.bn." in name or ".downsample.bn." in name:
        return 0.5
    return 1.0


def fill_synthetic_(module: torch.nn.Module, seed: int = WEIGHT_SEED, gains=None) -> torch.nn.Module:
    """Write the recipe into ``module`` (any module with the OTPose key set) in place.  When
    ``gains`` is None and the module carries a ``cfg`` (an OTPose), its calibrated gains are used."""
    if gains is None and getattr(module, "cfg", None) is not None:
        gains = gains_for(module.cfg)
    sd = module.state_dict()
    new = synthetic_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed, gains)
    with torch.no_grad():
        for k, v in new.items():
            sd[k].copy_(v.to(sd[k].dtype))
    return module


def synthetic_clip(batch: int, image_size, seed: int = INPUT_SEED, frames: int = 5):
    """``x`` (B, 15, H, W) ~ N(0, 1) (five ImageNet-normalised frames: cur, prev, next, pprev,
    nnext - reference script/Common.py:112-117) and ``margin`` (B, 4) float frame distances:
    [1, 1, 2, 2] with every fourth row [0, 1, 0, 2] (clip borders, reference
    dataset/PoseTrackDataset.py:263-293).  ``frames = 7`` (the configs[4] extension): (B, 21, H, W) and (B, 6) =
    [1, 1, 2, 2, 3, 3] / [0, 1, 0, 2, 0, 3]."""
    w, h = image_size
    r = (frames - 1) // 2
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    x = torch.randn((batch, 3 * frames, h, w), generator=gen, dtype=torch.float32)
    margin = torch.tensor([[float(k // 2 + 1) for k in range(2 * r)]]).repeat(batch, 1)
    margin[3::4] = torch.tensor([0.0 if k % 2 == 0 else float(k // 2 + 1) for k in range(2 * r)])
    return x, margin


def synthetic_targets(batch: int, heatmap_size, num_joints: int = 17, sigma: float = 3.0,
                      seed: int = INPUT_SEED + 1):
    """Gaussian target heatmaps with an exact 1.0 at each visible joint centre and a {0,1}
    ``target_weight`` (B, J, 1) with ~15 % zeros (reference utils/heatmap.py:48-105)."""
    w, h = heatmap_size
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    cx = torch.randint(0, w, (batch, num_joints), generator=gen)
    cy = torch.randint(0, h, (batch, num_joints), generator=gen)
    vis = (torch.rand((batch, num_joints), generator=gen) > 0.15).float()
    ys = torch.arange(h, dtype=torch.float32)[None, None, :, None]
    xs = torch.arange(w, dtype=torch.float32)[None, None, None, :]
    d2 = (xs - cx[..., None, None].float()) ** 2 + (ys - cy[..., None, None].float()) ** 2
    target = torch.exp(-d2 / (2 * sigma * sigma)) * vis[..., None, None]
    return target.contiguous(), vis[..., None].contiguous()


_SKELETON = (  # official PoseTrack joint order (right_ankle .. head_top): offsets in units of the person's size
    (-0.15, 1.0), (-0.15, 0.6), (-0.12, 0.2), (0.12, 0.2), (0.15, 0.6), (0.15, 1.0), (-0.45, 0.1), (-0.35, -0.15),
    (-0.22, -0.4), (0.22, -0.4), (0.35, -0.15), (0.45, 0.1), (0.0, -0.45), (0.0, -0.6), (0.0, -0.8))
_COCO_OF_OFFICIAL = (16, 14, 12, 11, 13, 15, 10, 8, 6, 5, 7, 9, 1, 0, 2)


def posetrack_eval_case(frames: int = 60, seed: int = 0, crowded=(), big_polygon=(), max_gt: int = 6, max_det: int = 8):
    """Seeded synthetic input of the PoseTrack evaluation (otpose_amd.posetrack_eval): poseval-format ground-truth frames
    with 0..max_gt persons (some with a subset of joints, a few rects without points, one with an empty point list), ignore
    polygons (convex and concave) in about every sixth frame, some covering a whole frame's ground truth, and in every sixth
    frame with two or more detections a box that swallows the first detection; and per frame
    0..max_det detections as ``(preds (N,17,3) float32 = x, y, maxval in the model's joint order, box (N,) float64,
    frame_id (N,) int64)``: jittered copies of ground-truth persons (pairs competing for one), and detections far from all.
    Frames of ``crowded`` hold 64 persons and 64 detections, frames of ``big_polygon`` a 64-vertex ignore polygon."""
    import numpy as np
    rng = np.random.default_rng(seed)
    skel = np.asarray(_SKELETON)
    crowded, big_polygon = set(crowded), set(big_polygon)
    gt_frames, preds, box, frame_id = [], [], [], []
    empty_points_done = False
    for f in range(frames):
        ng = 64 if f in crowded else int(rng.integers(0, max_gt + 1))
        nd = 64 if f in crowded else int(rng.integers(0, max_det + 1))
        poses, rects = [], []
        for _ in range(ng):
            c = rng.uniform((100, 100), (1820, 980))
            s = rng.uniform(60, 200)
            pose = c + skel * s + rng.normal(0, 0.02 * s, (15, 2))
            hs = s * rng.uniform(0.2, 0.3)
            poses.append((pose, hs))
            keep = np.ones(15, bool) if rng.random() < 0.6 else rng.random(15) < 0.6
            rect = {"x1": [float(c[0] - hs / 2)], "y1": [float(c[1] - 0.9 * s)], "x2": [float(c[0] + hs / 2)],
                    "y2": [float(c[1] - 0.9 * s + hs)], "track_id": [len(rects)]}
            u = rng.random()
            if u < 0.03 and f not in crowded:
                pass                                                   # a rect without annopoints: dropped by cleanupData
            elif u < 0.05 and not empty_points_done and f not in crowded:
                rect["annopoints"] = [{"point": []}]                   # stays: a person with no annotated joint
                empty_points_done = True
            else:
                rect["annopoints"] = [{"point": [{"id": [k], "x": [float(pose[k, 0])], "y": [float(pose[k, 1])]}
                                                 for k in range(15) if keep[k]]}]
            rects.append(rect)
        frame = {"annorect": rects}
        regions = []
        if f in big_polygon or rng.random() < 0.17:
            for _ in range(int(rng.integers(1, 3))):
                if poses and rng.random() < 0.7:
                    centre = poses[int(rng.integers(len(poses)))][0].mean(0) + rng.normal(0, 30, 2)
                else:
                    centre = rng.uniform((0, 0), (1920, 1080))
                nv = 64 if f in big_polygon else int(rng.integers(3, 13))
                radius = rng.uniform(40, 260)
                ang = np.sort(rng.uniform(0, 2 * np.pi, nv))
                rad = radius * (rng.uniform(0.35, 1.0, nv) if rng.random() < 0.5 else rng.uniform(0.9, 1.0, nv))
                regions.append(np.stack([centre[0] + rad * np.cos(ang), centre[1] + rad * np.sin(ang)], 1))
        if rng.random() < 0.04 and f not in crowded:                   # everything in the frame is ignored
            regions.append(np.array([[-4000.0, -4000.0], [6000.0, -4000.0], [6000.0, 5000.0], [-4000.0, 5000.0]]))
        gt_frames.append(frame)
        first_det = len(preds)
        for d in range(nd):
            det = np.empty((17, 3), np.float32)
            det[:, :2] = rng.uniform((0, 0), (1920, 1080), (17, 2))   # far from everything unless overwritten below
            u = rng.random()
            if poses and (u < 0.75 or f in crowded):
                # in a crowded frame detection d follows person d; else a random person (two may compete for one)
                pose, hs = poses[d % len(poses)] if f in crowded else poses[int(rng.integers(len(poses)))]
                sigma = (0.08, 0.25, 0.5)[int(rng.integers(3))] * 0.6 * hs * np.sqrt(2)
                det[list(_COCO_OF_OFFICIAL), :2] = pose + rng.normal(0, sigma, (15, 2))
            det[:, 2] = rng.uniform(0.05, 1.0, 17)
            preds.append(det)
            box.append(rng.uniform(0.3, 1.0))
            frame_id.append(f)
        if f % 6 == 1 and nd >= 2 and f not in crowded:
            # a box around the frame's FIRST detection (no random draw): that person loses every point while later ones stay
            q = preds[first_det][list(_COCO_OF_OFFICIAL), :2].astype(np.float64)
            (x0, y0), (x1, y1) = q.min(0) - 5.0, q.max(0) + 5.0
            regions.append(np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]]))
        if regions:
            frame["ignore_regions"] = [{"point": [{"x": [float(x)], "y": [float(y)]} for x, y in r]} for r in regions]
    preds = np.stack(preds) if preds else np.zeros((0, 17, 3), np.float32)
    return gt_frames, preds.astype(np.float32), np.asarray(box, np.float64), np.asarray(frame_id, np.int64)


def pose_nms_case(frames: int = 300, seed: int = 0, low_vis: float = 0.05):
    """Seeded synthetic input of the pose NMS (``ops.pose_nms``, ``posetrack_eval.PoseNMS``): :func:`posetrack_eval_case`
    (one frame of 64 and one of 63 detections) with what a detector adds - jittered duplicates (0.5-20 px, lower box score)
    of about every second detection - and one frame each for the special persons, named in the returned ``special`` dict by
    sample index: ``exact`` (a copy of ``exact_of``: OKS 1), ``low_vis`` (every maxval below ``low_vis``), ``zero_area`` (a
    copy of ``zero_area_of`` with area 0), ``equal`` (the person score of ``equal_of``, bit for bit, another pose),
    ``nan_xy`` (NaN coordinates) and ``nan_score`` (a NaN box score), the last two in frames without another special person.
    Returns ``(gt_frames, preds (N,17,3) float32, box (N,) float64, frame_id (N,) int64, area (N,) float64, special)``."""
    import numpy as np
    gt_frames, preds, box, fid = posetrack_eval_case(frames, seed, crowded=(5, frames // 2))
    rng = np.random.default_rng([seed, 0x4e4d53])
    last = np.nonzero(fid == frames // 2)[0][-1]                       # 64 -> 63 detections in the second crowded frame
    preds, box, fid = np.delete(preds, last, 0), np.delete(box, last), np.delete(fid, last)
    span = preds[:, :, :2].max(1).astype(np.float64) - preds[:, :, :2].min(1).astype(np.float64)
    area = span.prod(1) * 1.25 ** 2 * rng.uniform(0.9, 1.1, fid.size)
    count = np.bincount(fid, minlength=frames)
    new_p, new_b, new_f, new_a = [], [], [], []

    def add(src, jitter, frame=None):
        det = preds[src].copy()
        det[:, :2] += rng.normal(0, jitter, (17, 2)).astype(np.float32) if jitter else 0
        new_p.append(det)
        new_b.append(box[src] * rng.uniform(0.5, 0.95))
        new_f.append(fid[src] if frame is None else frame)
        new_a.append(area[src] * rng.uniform(0.9, 1.1))
        return fid.size + len(new_p) - 1

    for s in np.nonzero((count[fid] < 20) & (rng.random(fid.size) < 0.5))[0]:
        for _ in range(int(rng.integers(1, 3))):
            add(s, rng.uniform(0.5, 20.0))
    # the special persons: one frame each, among the frames that are evaluated and hold 2..8 detections
    plain = [f for f in range(frames) if 2 <= count[f] <= 8 and len(gt_frames[f]["annorect"]) > 0
             and any("annopoints" in r for r in gt_frames[f]["annorect"])]
    chosen = rng.choice(plain, 6, replace=False)
    first = [int(np.nonzero(fid == f)[0][0]) for f in chosen]
    special = {"exact_of": first[0], "exact": add(first[0], 0.0)}
    special["low_vis"] = add(first[1], 3.0)
    new_p[-1][:, 2] = rng.uniform(0.2, 0.8, 17).astype(np.float32) * np.float32(low_vis)
    special["zero_area_of"], special["zero_area"] = first[2], add(first[2], 0.0)
    new_a[-1] = 0.0
    special["equal_of"], special["equal"] = first[3], add(first[3], 0.0)
    new_p[-1][:, :2] += rng.uniform(150.0, 300.0, 2).astype(np.float32)
    new_b[-1] = box[first[3]]
    special["nan_xy"] = add(first[4], 2.0)
    new_p[-1][3:6, :2] = np.nan
    special["nan_score"] = add(first[5], 40.0)
    new_b[-1] = np.nan
    preds = np.concatenate([preds, np.stack(new_p)]).astype(np.float32)
    return (gt_frames, preds, np.concatenate([box, new_b]), np.concatenate([fid, np.asarray(new_f, np.int64)]),
            np.concatenate([area, new_a]), special)
