"""Temporal segment NMS (csrc/segnms.hip; the reference's thirdparty/utils nms_1d_cpu; drop-in names in segnms.py) and
temporal detection AP (csrc/segap.hip; the reference's thirdparty/utils/metrics.py; drop-in names in segmetrics.py)."""
from __future__ import annotations

import ctypes

import torch

from .. import hip
from .base import _K, check_f32, require_gpu, _launch


def _seg_batch(segs, scores, offsets):
    """Checked contiguous ``(segs (N, 2) f32, scores (N) f32, offsets (G+1) i32)`` of a segmented batch, N >= 1 and G >= 1."""
    require_gpu(segs, scores, offsets)
    check_f32(segs, scores)
    if segs.dim() != 2 or segs.shape[1] != 2 or scores.dim() != 1 or scores.shape[0] != segs.shape[0] or segs.shape[0] < 1:
        raise ValueError(f"segs must be (N, 2) and scores (N) with N >= 1, got {tuple(segs.shape)} and {tuple(scores.shape)}")
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.shape[0] < 2:
        raise ValueError("offsets must be a (G + 1) int32 tensor with G >= 1")
    return segs.contiguous(), scores.contiguous(), offsets.contiguous()


def _seg_workspace(g, n, device, workspace):
    need = hip.lib().otp_seg_nms_workspace(g, n)
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.int32, device=device)
    return workspace, workspace.numel() * workspace.element_size()


def seg_nms(segs, scores, offsets, iou_threshold, min_score=0.0, max_num=0, workspace=None):
    """Hard 1-D NMS (``nms_1d_cpu``, nms_cpu.cpp:19-58, behind ``NMSop``'s ``scores > min_score`` filter) of every group of a
    segmented batch in one launch: group g is rows ``offsets[g] .. offsets[g + 1]`` of ``segs`` (N, 2) / ``scores`` (N).
    Returns device tensors ``(counts (G,) int32, keep (N,) int32)``: rows ``offsets[g] ..`` of ``keep`` hold the group's kept
    indices (relative to its first row) in descending-score order, cut at ``max_num`` when it is > 0, then -1."""
    segs, scores, offsets = _seg_batch(segs, scores, offsets)
    g, n, dev = offsets.shape[0] - 1, segs.shape[0], segs.device
    workspace, nbytes = _seg_workspace(g, n, dev, workspace)
    counts = torch.empty(g, dtype=torch.int32, device=dev)
    keep = torch.empty(n, dtype=torch.int32, device=dev)
    _launch(hip.lib().otp_seg_nms, "otp_seg_nms",
            (hip.ptr(segs), hip.ptr(scores), hip.ptr(offsets), g, n, float(iou_threshold), float(min_score), int(max_num),
             hip.ptr(workspace), nbytes, hip.ptr(counts), hip.ptr(keep)), segs)
    return counts, keep


def seg_softnms(segs, scores, offsets, iou_threshold, sigma=0.5, min_score=0.0, method=2, max_num=0, workspace=None):
    """Soft 1-D NMS (``softnms_1d_cpu``, nms_cpu.cpp:67-160; ``method`` 0 hard, 1 linear, 2 gaussian) of every group of a
    segmented batch in one launch.  Returns device tensors ``(counts (G,) int32, dets (N, 3) float32, inds (N,) int32)``: rows
    ``offsets[g] + r`` hold the ``(x1, x2, decayed score)`` and the group-relative index of the segment taken in round r,
    cut at ``max_num`` when it is > 0; the group's remaining rows hold zeros and -1."""
    segs, scores, offsets = _seg_batch(segs, scores, offsets)
    if int(method) not in (0, 1, 2):
        raise ValueError(f"method must be 0 (hard), 1 (linear) or 2 (gaussian), got {method}")
    g, n, dev = offsets.shape[0] - 1, segs.shape[0], segs.device
    workspace, nbytes = _seg_workspace(g, n, dev, workspace)
    counts = torch.empty(g, dtype=torch.int32, device=dev)
    dets = torch.empty((n, 3), dtype=torch.float32, device=dev)
    inds = torch.empty(n, dtype=torch.int32, device=dev)
    _launch(hip.lib().otp_seg_softnms, "otp_seg_softnms",
            (hip.ptr(segs), hip.ptr(scores), hip.ptr(offsets), g, n, float(iou_threshold), float(sigma), float(min_score),
             int(method), int(max_num), hip.ptr(workspace), nbytes, hip.ptr(counts), hip.ptr(dets), hip.ptr(inds)), segs)
    return counts, dets, inds


def seg_voting_groups(nms_segs, nms_offsets, segs, scores, offsets, voting_thresh):
    """``seg_voting`` (nms.py:67-101) for the kept segments ``nms_segs`` (K, 2) of every group (``nms_offsets`` (G+1) int32)
    against all segments of the same group of the batch ``segs`` / ``scores`` / ``offsets``: (K, 2) score-weighted means of
    the segments with ``iou >= voting_thresh``; a row without such a segment is NaN, as in the reference."""
    segs, scores, offsets = _seg_batch(segs, scores, offsets)
    require_gpu(nms_segs, nms_offsets)
    check_f32(nms_segs)
    if nms_segs.dim() != 2 or nms_segs.shape[1] != 2:
        raise ValueError(f"nms_segs must be (K, 2), got {tuple(nms_segs.shape)}")
    if nms_offsets.dtype != torch.int32 or nms_offsets.shape != offsets.shape:
        raise ValueError("nms_offsets must be a (G + 1) int32 tensor like offsets")
    nms_segs, nms_offsets = nms_segs.contiguous(), nms_offsets.contiguous()
    k = nms_segs.shape[0]
    out = torch.empty((k, 2), dtype=torch.float32, device=segs.device)
    if k:
        _launch(hip.lib().otp_seg_voting, "otp_seg_voting",
                (hip.ptr(nms_segs), hip.ptr(nms_offsets), hip.ptr(segs), hip.ptr(scores), hip.ptr(offsets),
                 offsets.shape[0] - 1, k, segs.shape[0], float(voting_thresh), hip.ptr(out)), segs)
    return out


# ------------------------------------------------------------------------------------------------
# temporal detection AP (csrc/segap.hip; the reference's thirdparty/utils/metrics.py); the drop-in names are in segmetrics.py
# ------------------------------------------------------------------------------------------------
def _check_i32(what, t, min_len):
    if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < min_len:
        raise ValueError(f"{what} must be a 1-D int32 tensor of at least {min_len} entries")
    return t.contiguous()


def seg_ap_match(pred_seg, pred_offsets, gt_seg, gt_offsets, thresholds, workspace=None):
    """The greedy assignment of ``compute_average_precision_detection`` (metrics.py:243-271) for every (video, class) group
    and every tIoU threshold in one launch.  Group g is rows ``pred_offsets[g] .. pred_offsets[g + 1]`` of ``pred_seg`` (N, 2)
    float64, already in descending-score order inside the group, and rows ``gt_offsets[g] .. gt_offsets[g + 1]`` of ``gt_seg``
    (M, 2) float64.  ``thresholds``: up to ``OTP_SEG_AP_MAX_THRESHOLDS`` host floats.  Returns the device tensor ``match``
    (T, N) int32: the matched ground truth's row relative to the group's first, or -1 for a false positive."""
    require_gpu(pred_seg, pred_offsets, gt_seg, gt_offsets)
    for what, t in (("pred_seg", pred_seg), ("gt_seg", gt_seg)):
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 2:
            raise ValueError(f"{what} must be an (n, 2) float64 tensor, got {tuple(t.shape)} {t.dtype}")
    pred_offsets, gt_offsets = _check_i32("pred_offsets", pred_offsets, 2), _check_i32("gt_offsets", gt_offsets, 2)
    if pred_offsets.shape != gt_offsets.shape:
        raise ValueError("pred_offsets and gt_offsets must describe the same G groups")
    thr = [float(v) for v in thresholds]
    t, n, m, g, dev = len(thr), pred_seg.shape[0], gt_seg.shape[0], pred_offsets.shape[0] - 1, pred_seg.device
    if not 1 <= t <= _K["OTP_SEG_AP_MAX_THRESHOLDS"]:
        raise ValueError(f"1 .. {_K['OTP_SEG_AP_MAX_THRESHOLDS']} thresholds, got {t}")
    if n == 0 or m == 0:                              # nothing to match: every prediction is a false positive
        return torch.full((t, n), -1, dtype=torch.int32, device=dev)
    need = hip.lib().otp_seg_ap_match_workspace(g, m, t)
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.int32, device=dev)
    match = torch.empty((t, n), dtype=torch.int32, device=dev)
    pred_seg, gt_seg = pred_seg.contiguous(), gt_seg.contiguous()
    _launch(hip.lib().otp_seg_ap_match, "otp_seg_ap_match",
            (hip.ptr(pred_seg), hip.ptr(pred_offsets), hip.ptr(gt_seg), hip.ptr(gt_offsets),
             (ctypes.c_double * t)(*thr), g, n, m, t, hip.ptr(workspace), workspace.numel() * workspace.element_size(),
             hip.ptr(match)), pred_seg)
    return match


def seg_ap(match, order, class_offsets, npos):
    """Interpolated AP (metrics.py:273-282, 312-321) of every (threshold, class) from ``match`` (T, N) int32 of
    :func:`seg_ap_match`.  ``order`` (N) int32: the rows of ``match`` in class-major order, descending score inside a class;
    ``class_offsets`` (C+1) int32 over ``order``; ``npos`` (C) int32: the ground truths of each class.  Returns ``ap`` (T, C)
    float64 on the device; a class without predictions gets 0."""
    require_gpu(match, order, class_offsets, npos)
    if match.dtype != torch.int32 or match.dim() != 2:
        raise ValueError("match must be a (T, N) int32 tensor")
    t, n = match.shape
    order, class_offsets = _check_i32("order", order, 0), _check_i32("class_offsets", class_offsets, 2)
    c = class_offsets.shape[0] - 1
    npos = _check_i32("npos", npos, c)
    if order.shape[0] != n or npos.shape[0] != c or not 1 <= t <= _K["OTP_SEG_AP_MAX_THRESHOLDS"]:
        raise ValueError(f"order must have N = {n} entries, npos C = {c}, and T must be 1 .. {_K['OTP_SEG_AP_MAX_THRESHOLDS']}")
    if n == 0:
        return torch.zeros((t, c), dtype=torch.float64, device=match.device)
    ap = torch.empty((t, c), dtype=torch.float64, device=match.device)
    match = match.contiguous()
    _launch(hip.lib().otp_seg_ap, "otp_seg_ap",
            (hip.ptr(match), hip.ptr(order), hip.ptr(class_offsets), hip.ptr(npos), c, t, n, hip.ptr(ap)), match)
    return ap
