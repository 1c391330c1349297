"""Temporal segment NMS on the GPU: the names and call signatures of the reference's ``thirdparty/utils/nms.py``
(``NMSop``, ``SoftNMSop``, ``seg_voting``, ``batched_nms``) over the kernels of csrc/segnms.hip, and
``batched_nms_videos`` for many videos in one launch.

Every (video, class) pair is one group of a segmented batch: the segments are sorted by group on the device, the group
offsets come from the run lengths of the sorted keys, and one launch (one workgroup per group) serves them all - no Python
loop over ``torch.unique``.  Results stay on the input's device (the reference returns CPU tensors).  CPU tensors raise
``NotImplementedError``, like every operator here.  The lengths of the results depend on the data, so a call ends with a
host synchronisation, as any NMS that returns a tensor of kept rows does.
"""
from __future__ import annotations

import torch

from . import ops

__all__ = ["NMSop", "SoftNMSop", "seg_voting", "batched_nms", "batched_nms_videos"]


def _offsets(lengths, device):
    """(G + 1) int32 offsets of groups with the given lengths (a 1-D device tensor of any integer type)."""
    off = torch.zeros(lengths.shape[0] + 1, dtype=torch.int32, device=device)
    off[1:] = torch.cumsum(lengths, 0)
    return off


def _rows(counts, offsets):
    """Flat rows ``offsets[g] + r, r < counts[g]`` of every group in group order, and the group of each."""
    n_groups = counts.shape[0]
    lengths = (offsets[1:] - offsets[:-1]).long()
    group = torch.repeat_interleave(torch.arange(n_groups, device=counts.device), lengths)
    pos = torch.arange(group.shape[0], device=counts.device)
    valid = (pos - offsets[:-1].long()[group]) < counts.long()[group]
    return pos[valid], group[valid]


def _whole(segs):
    return torch.tensor([0, segs.shape[0]], dtype=torch.int32, device=segs.device)


def _check(segs, scores, cls_idxs=None):
    ops.require_gpu(segs, scores, cls_idxs)
    ops.check_f32(segs, scores)


def _empty(segs, cls_idxs):
    """The reference's answer to an input without segments (nms.py:119-122), on the input's device."""
    return (torch.zeros([0, 2], device=segs.device), torch.zeros([0], device=segs.device),
            torch.zeros([0], dtype=cls_idxs.dtype, device=segs.device))


class NMSop(torch.autograd.Function):
    """``NMSop.apply(segs, cls_idxs, scores, iou_threshold, min_score, max_num)`` of nms.py:8-35: the kept segments, scores
    and classes in descending-score order."""

    @staticmethod
    def forward(ctx, segs, cls_idxs, scores, iou_threshold, min_score, max_num):
        if segs.shape[0] == 0:
            return segs.clone(), scores.clone(), cls_idxs.clone()
        _check(segs, scores, cls_idxs)
        counts, keep = ops.seg_nms(segs, scores, _whole(segs), iou_threshold, min_score, max_num)
        inds = keep[:int(counts[0])].long()
        return segs[inds], scores[inds], cls_idxs[inds]


class SoftNMSop(torch.autograd.Function):
    """``SoftNMSop.apply(segs, scores, cls_idxs, iou_threshold, sigma, min_score, method, max_num)`` of nms.py:38-64: the
    segments in the order they were taken, with their decayed scores."""

    @staticmethod
    def forward(ctx, segs, scores, cls_idxs, iou_threshold, sigma, min_score, method, max_num):
        if segs.shape[0] == 0:
            return segs.clone(), scores.clone(), cls_idxs.clone()
        _check(segs, scores, cls_idxs)
        counts, dets, inds = ops.seg_softnms(segs, scores, _whole(segs), iou_threshold, sigma, min_score, method, max_num)
        k = int(counts[0])
        return dets[:k, :2].clone(), dets[:k, 2].clone(), cls_idxs[inds[:k].long()]


def seg_voting(nms_segs, all_segs, all_scores, iou_threshold, score_offset=1.5):
    """nms.py:67-101: every kept segment becomes the score-weighted mean of all segments with ``iou >= iou_threshold``.
    ``score_offset`` is accepted and unused: the reference computes ``all_scores + score_offset`` and weighs by the raw
    scores."""
    _check(nms_segs, all_scores)
    _check(all_segs, all_scores)
    if nms_segs.shape[0] == 0 or all_segs.shape[0] == 0:
        return torch.zeros((nms_segs.shape[0], 2), dtype=torch.float32, device=nms_segs.device)   # a product over no terms
    nms_off = torch.tensor([0, nms_segs.shape[0]], dtype=torch.int32, device=nms_segs.device)
    return ops.seg_voting_groups(nms_segs, nms_off, all_segs, all_scores, _whole(all_segs), iou_threshold)


def batched_nms_videos(videos, iou_threshold, min_score, max_seg_num, use_soft_nms=True, multiclass=True, sigma=0.5,
                       voting_thresh=0.75):
    """``batched_nms`` for a list of videos ``(segs (N_v, 2), scores (N_v), cls_idxs (N_v))`` in one launch: returns the
    list of the triples ``batched_nms`` returns for each.  All tensors on one device."""
    videos = list(videos)
    if not videos:
        return []
    results = [None] * len(videos)
    filled = [v for v, (segs, _, _) in enumerate(videos) if segs.shape[0] > 0]
    for v, (segs, scores, cls) in enumerate(videos):
        if segs.shape[0] == 0:
            results[v] = _empty(segs, cls)            # no kernel runs: answered wherever the tensors are
        else:
            _check(segs, scores, cls)
    if not filled:
        return results
    dev = videos[filled[0]][0].device
    segs = torch.cat([videos[v][0] for v in filled])
    scores = torch.cat([videos[v][1] for v in filled])
    cls = torch.cat([videos[v][2] for v in filled])
    lengths = torch.tensor([videos[v][0].shape[0] for v in filled], device=dev)
    vid = torch.repeat_interleave(torch.arange(len(filled), device=dev), lengths)

    if multiclass:
        # one group per (video, class): a stable sort by the pair keeps the input order inside a group, as the reference's
        # torch.where(cls_idxs == class_id) does, and orders the groups of a video by ascending class, as torch.unique does
        lo = cls.min()
        span = cls.max() - lo + 1
        key = vid * span.long() + (cls - lo).long()
        key, perm = torch.sort(key, stable=True)
        segs_g, scores_g, cls_g = segs[perm].contiguous(), scores[perm].contiguous(), cls[perm]
        groups, group_len = torch.unique_consecutive(key, return_counts=True)
        offsets = _offsets(group_len, dev)
        group_vid = torch.div(groups, span.long(), rounding_mode="floor")
    else:
        segs_g, scores_g, cls_g = segs.contiguous(), scores.contiguous(), cls
        offsets = _offsets(lengths, dev)
        group_vid = torch.arange(len(filled), device=dev)

    if use_soft_nms:
        counts, dets, inds = ops.seg_softnms(segs_g, scores_g, offsets, iou_threshold, sigma, min_score, 2, max_seg_num)
        rows, group = _rows(counts, offsets)
        new_segs, new_scores = dets[rows, :2], dets[rows, 2]
        new_cls = cls_g[inds[rows].long() + offsets[:-1].long()[group]]
    else:
        counts, keep = ops.seg_nms(segs_g, scores_g, offsets, iou_threshold, min_score, max_seg_num)
        rows, group = _rows(counts, offsets)
        src = keep[rows].long() + offsets[:-1].long()[group]
        new_segs, new_scores, new_cls = segs_g[src], scores_g[src], cls_g[src]
    if not multiclass and voting_thresh > 0 and new_segs.shape[0] > 0:
        new_segs = ops.seg_voting_groups(new_segs, _offsets(counts.long(), dev), segs_g, scores_g, offsets, voting_thresh)

    # per video: descending score, cut at max_seg_num (a stable sort by video over the score order)
    out_vid = group_vid[group]
    by_score = torch.sort(new_scores, descending=True, stable=True)[1]
    order = by_score[torch.sort(out_vid[by_score], stable=True)[1]]
    per_video = torch.bincount(out_vid, minlength=len(filled))
    start = torch.cumsum(per_video, 0) - per_video
    sorted_vid = out_vid[order]
    order = order[(torch.arange(order.shape[0], device=dev) - start[sorted_vid]) < max_seg_num]
    sizes = torch.clamp(per_video, max=max_seg_num).tolist()
    pieces = zip(torch.split(new_segs[order], sizes), torch.split(new_scores[order], sizes), torch.split(new_cls[order], sizes))
    for v, piece in zip(filled, pieces):
        results[v] = piece
    return results


def batched_nms(segs, scores, cls_idxs, iou_threshold, min_score, max_seg_num, use_soft_nms=True, multiclass=True, sigma=0.5,
                voting_thresh=0.75):
    """nms.py:104-191 on the GPU: per-class (``multiclass``) or class-agnostic NMS, soft (gaussian) or hard; segment voting on
    the class-agnostic path when ``voting_thresh > 0``; then descending score and the ``max_seg_num`` cut.  Returns
    ``(segs (K, 2), scores (K), cls_idxs (K))`` on the input's device."""
    return batched_nms_videos([(segs, scores, cls_idxs)], iou_threshold, min_score, max_seg_num, use_soft_nms, multiclass,
                              sigma, voting_thresh)[0]
