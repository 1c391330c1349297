"""PoseTrack evaluation on the device: pose-to-GT assignment, AP and pose NMS (csrc/poseval.hip, csrc/posenms.hip)."""
from __future__ import annotations

import ctypes
import math

import torch

from .. import hip
from .base import _K, _tensor_arg

POSEVAL_JOINTS, POSEVAL_MAX_PR, POSEVAL_MAX_GT = _K["OTP_POSEVAL_JOINTS"], _K["OTP_POSEVAL_MAX_PR"], _K["OTP_POSEVAL_MAX_GT"]


def pose_assign(pr_off, pr_sample, preds, maxvals, box_score, gt_off, gt_xy, gt_has, gt_head, poly_off, vert_off, vert_xy,
                dist_thresh=0.5):
    """Device form of reference utils/evaluate.py:22-67 + 467-682 (removeIgnoredPoints, assignGTmulti) over CSR-packed
    frames, one launch (``otp_pose_assign``; layout in include/otpose_hip.h, packing in ``posetrack_eval``).  Returns
    ``(labels (NP,15) int8, scores (NP,15) float64, ngt (F,15) int32)``: label 1 match, 0 false positive, -1 no entry.
    Raises ``ValueError`` for a frame with more than ``POSEVAL_MAX_PR`` predicted or ``POSEVAL_MAX_GT`` ground-truth
    persons or a sample index outside ``preds`` (the offsets are read back for the check: this is evaluation plumbing, it
    synchronises)."""
    i32, f64 = torch.int32, torch.float64
    pr_off = _tensor_arg(pr_off, i32, (None,), "pr_off")
    f = pr_off.numel() - 1
    pr_sample = _tensor_arg(pr_sample, i32, (None,), "pr_sample")
    preds = _tensor_arg(preds, torch.float32, (None, 17, 2), "preds")
    n = preds.shape[0]
    if torch.is_tensor(maxvals) and maxvals.dim() == 2:
        maxvals = maxvals.unsqueeze(-1)
    maxvals = _tensor_arg(maxvals, torch.float32, (n, 17, 1), "maxvals")
    box_score = _tensor_arg(box_score, f64, (n,), "box_score")
    gt_off = _tensor_arg(gt_off, i32, (f + 1,), "gt_off")
    gt_xy = _tensor_arg(gt_xy, f64, (None, POSEVAL_JOINTS, 2), "gt_xy")
    ng = gt_xy.shape[0]
    gt_has = _tensor_arg(gt_has, i32, (ng,), "gt_has")
    gt_head = _tensor_arg(gt_head, f64, (ng, 4), "gt_head")
    poly_off = _tensor_arg(poly_off, i32, (f + 1,), "poly_off")
    vert_off = _tensor_arg(vert_off, i32, (None,), "vert_off")
    vert_xy = _tensor_arg(vert_xy, f64, (None, 2), "vert_xy")
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
    labels_sorted = _tensor_arg(labels_sorted, torch.int8, (None,), "labels_sorted")
    joint_off = _tensor_arg(joint_off, torch.int64, (None,), "joint_off")
    j = joint_off.numel() - 1
    n_gt = _tensor_arg(n_gt, torch.int64, (j,), "n_gt")
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
    pr_off = _tensor_arg(pr_off, i32, (None,), "pr_off")
    f = pr_off.numel() - 1
    pr_sample = _tensor_arg(pr_sample, i32, (None,), "pr_sample")
    preds = _tensor_arg(preds, torch.float32, (None, 17, 2), "preds")
    n = preds.shape[0]
    if torch.is_tensor(maxvals) and maxvals.dim() == 2:
        maxvals = maxvals.unsqueeze(-1)
    maxvals = _tensor_arg(maxvals, torch.float32, (n, 17, 1), "maxvals")
    box_score = _tensor_arg(box_score, f64, (n,), "box_score")
    area = _tensor_arg(area, f64, (n,), "area")
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
