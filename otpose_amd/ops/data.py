"""Data preparation on the device: frames to clips, person crops, heat-map targets, the crop plan."""
from __future__ import annotations

import collections
import math

import torch

from .. import hip
from .base import require_gpu, _tensor_arg

IMAGENET_MEAN = (0.485, 0.456, 0.406)        # utils/transform.py:7-8
IMAGENET_STD = (0.229, 0.224, 0.225)


def frames_to_clip(frames_u8, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """uint8 RGB frames (B, F, H, W, 3) (the five warped crops of dataset/PoseTrackDataset.py:390-399) -> the model input
    (B, 3F, H, W) float32: ToTensor + Normalize per frame (utils/transform.py:11-15) and the channel concat of
    script/Common.py:117 in one kernel, bit-identical to the torchvision float32 arithmetic.  Moves 4x fewer bytes over
    PCIe than shipping normalised floats."""
    require_gpu(frames_u8)
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
    require_gpu(pool)
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
    from ..crop import gaussian_table
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
    # type, then shape, then (below) device: every argument error shows without a GPU
    boxes = _tensor_arg(boxes, torch.float64, (None, None, 4), "boxes", on_gpu=False)
    s, k = boxes.shape[:2]
    scores = _tensor_arg(scores, torch.float32, (s, k), "scores", on_gpu=False)
    counts = _tensor_arg(counts, i32, (s,), "counts", on_gpu=False)
    frame_number = _tensor_arg(frame_number, i32, (s,), "frame_number", on_gpu=False)
    num_frames = _tensor_arg(num_frames, i32, (s,), "num_frames", on_gpu=False)
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
    require_gpu(*tensors)
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
