"""Float64 restatement of the reference's temporal detection metric (thirdparty/utils/metrics.py: ``segment_iou``,
``compute_average_precision_detection``, ``interpolated_prec_rec``, ``ANETdetection.evaluate``) and of
``postprocess_results`` (thirdparty/utils/postprocessing.py), in numpy, on dicts of columns instead of data frames.
tests/golden/make_golden_segap.py asserts that it reproduces the reference's ``ap`` bit for bit on every recorded case: both
evaluate the same numpy expressions on the same float64 values.

Besides the numbers it returns what the reference keeps to itself: the ``match`` table (per threshold and prediction the row
of the matched ground truth inside its (video, class) group, or -1) and the true-positive flags.

Decisions the reference leaves open are closed here as the kernels close them: exactly equal scores are ordered by input row,
exactly equal tIoUs by ground-truth row, a NaN tIoU orders above every number (where numpy's ``argsort()[::-1]`` puts it).

``margins``: a dict that receives the smallest distance of every discrete decision from its alternative: ``score`` (smallest gap
of two scores inside a class), ``tiou`` (smallest gap of two positive tIoUs of one prediction), ``thr`` (smallest
|tIoU - threshold|).
"""
from __future__ import annotations

import numpy as np


def _note(margins, key, value):
    if margins is not None and value == value:
        margins[key] = min(margins.get(key, np.inf), float(value))


def segment_iou(target, candidates):
    """tIoU of one segment (2,) with each of (n, 2) segments, float64."""
    lo = np.maximum(target[0], candidates[:, 0])
    hi = np.minimum(target[1], candidates[:, 1])
    inter = (hi - lo).clip(0)
    union = (candidates[:, 1] - candidates[:, 0]) + (target[1] - target[0]) - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter.astype(float) / union


def ranked(tiou):
    """Ground-truth rows by descending tIoU: NaN first, equal values by ascending row."""
    key = np.where(np.isnan(tiou), np.inf, tiou)
    return np.argsort(-key, kind="stable")


def match_group(pred_seg, gt_seg, thresholds, margins=None):
    """(T, n) int32 matches of one group's predictions (n, 2), given in descending-score order, to its ground truths (m, 2)."""
    T, n, m = len(thresholds), len(pred_seg), len(gt_seg)
    match = np.full((T, n), -1, np.int32)
    if m == 0:
        return match
    locked = np.zeros((T, m), bool)
    thr = np.asarray(thresholds, np.float64)
    for p in range(n):
        tiou = segment_iou(pred_seg[p], gt_seg)
        if margins is not None:
            pos = np.sort(tiou[tiou > 0])
            if len(pos) > 1:
                _note(margins, "tiou", np.diff(pos).min())
            fin = tiou[~np.isnan(tiou)]
            if len(fin):
                _note(margins, "thr", np.abs(fin[:, None] - thr[None, :]).min())
        order = ranked(tiou)
        for t in range(T):
            for j in order:
                if tiou[j] < thr[t]:
                    break
                if not locked[t, j]:
                    locked[t, j] = True
                    match[t, p] = j
                    break
    return match


def match_groups(pred_seg, pred_offsets, gt_seg, gt_offsets, thresholds, margins=None):
    """(T, N) int32: ``match_group`` of every group of a segmented batch (what ``ops.seg_ap_match`` returns)."""
    out = np.full((len(thresholds), len(pred_seg)), -1, np.int32)
    for g in range(len(pred_offsets) - 1):
        p0, p1, q0, q1 = pred_offsets[g], pred_offsets[g + 1], gt_offsets[g], gt_offsets[g + 1]
        out[:, p0:p1] = match_group(pred_seg[p0:p1], gt_seg[q0:q1], thresholds, margins)
    return out


def interpolated_ap(prec, rec):
    """VOC 2011: precision made non-increasing from the right, summed over the steps of recall."""
    mprec = np.hstack([[0], prec, [0]])
    mrec = np.hstack([[0], rec, [1]])
    for i in range(len(mprec) - 2, -1, -1):
        mprec[i] = max(mprec[i], mprec[i + 1])
    idx = np.where(mrec[1:] != mrec[:-1])[0] + 1
    return np.sum((mrec[idx] - mrec[idx - 1]) * mprec[idx])


def ap_from_tp(tp, npos):
    """(T,) AP from the (T, n) true-positive flags of a class's predictions in descending-score order."""
    tp = tp.astype(np.float64)
    tp_cum = np.cumsum(tp, axis=1).astype(float)
    fp_cum = np.cumsum(1.0 - tp, axis=1).astype(float)
    rec = tp_cum / float(npos)
    prec = tp_cum / (tp_cum + fp_cum)
    return np.array([interpolated_ap(prec[t], rec[t]) for t in range(tp.shape[0])])


def class_ap(gt_vid, gt_seg, pred_vid, pred_seg, pred_score, thresholds, margins=None):
    """One class: ``(ap (T,), match (T, n), tp (T, n) bool, order (n,))``.  ``order``: the prediction rows in descending
    score; ``match`` and ``tp`` are in that order, ``match`` relative to the ground truths of the prediction's video in
    their input order."""
    T, n = len(thresholds), len(pred_score)
    if len(gt_vid) == 0:
        raise ValueError("a class without ground truth")
    order = np.argsort(-np.asarray(pred_score, np.float64), kind="stable")
    if margins is not None and n > 1:
        _note(margins, "score", np.diff(np.sort(np.asarray(pred_score, np.float64))).min())
    match = np.full((T, n), -1, np.int32)
    rows_of = {}
    for r, v in enumerate(gt_vid):
        rows_of.setdefault(v, []).append(r)
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    by_video = {}
    for i in order:
        by_video.setdefault(pred_vid[i], []).append(i)
    for v, rows in by_video.items():
        if v in rows_of:
            rows = np.array(rows)
            match[:, pos[rows]] = match_group(pred_seg[rows], gt_seg[np.array(rows_of[v])], thresholds, margins)
    tp = match >= 0
    ap = ap_from_tp(tp, len(gt_vid)) if n else np.zeros(T)
    return ap, match, tp, order


def remap(labels, gt_labels):
    """``(index, keep)``: the position of each label among the sorted distinct ground-truth labels; ``keep`` False for a label
    that is not one of them (such predictions are dropped)."""
    gt_labels = np.asarray(gt_labels)
    index = np.minimum(np.searchsorted(gt_labels, labels), len(gt_labels) - 1)
    return index, gt_labels[index] == labels


def detection_ap(gt, preds, thresholds, margins=None):
    """``ANETdetection.evaluate`` on tables (dicts of columns): ``(ap (T, C), mAP (T,), average_mAP)``."""
    gt_labels = np.unique(gt["label"])
    gt_cls, _ = remap(np.asarray(gt["label"]), gt_labels)
    cls, keep = remap(np.asarray(preds["label"]), gt_labels)
    gt_vid, pred_vid = np.asarray(gt["video-id"], dtype=object), np.asarray(preds["video-id"], dtype=object)
    gt_seg = np.stack([gt["t-start"], gt["t-end"]], 1).astype(np.float64)
    pred_seg = np.stack([preds["t-start"], preds["t-end"]], 1).astype(np.float64)
    score = np.asarray(preds["score"], np.float64)
    ap = np.zeros((len(thresholds), len(gt_labels)))
    for c in range(len(gt_labels)):
        g, p = gt_cls == c, keep & (cls == c)
        if p.any():
            ap[:, c] = class_ap(gt_vid[g], gt_seg[g], pred_vid[p], pred_seg[p], score[p], thresholds, margins)[0]
    mAP = ap.mean(axis=1)
    return ap, mAP, mAP.mean()


def kernel_tables(gt, preds, thresholds, margins=None):
    """What the two kernels read and write for ``detection_ap(gt, preds, thresholds)``, laid out as otpose_amd/segmetrics.py
    lays it out: groups ``video * C + class`` over the ground truth's videos in order of first appearance plus one video
    that stands for every other; predictions with a label outside the ground truth dropped.  Returns a dict with
    ``pred_seg``, ``pred_offsets``, ``gt_seg``, ``gt_offsets``, ``match`` (T, N), ``order``, ``class_offsets``, ``npos`` and
    ``ap`` (T, C), the last from ``ap_from_tp`` of every class."""
    gt_labels = np.unique(gt["label"])
    C = len(gt_labels)
    number = {}
    for v in gt["video-id"]:
        number.setdefault(v, len(number))
    G = (len(number) + 1) * C
    gt_cls, _ = remap(np.asarray(gt["label"]), gt_labels)
    gt_key = np.array([number[v] for v in gt["video-id"]], np.int64) * C + gt_cls
    perm = np.argsort(gt_key, kind="stable")
    gt_seg = np.stack([gt["t-start"], gt["t-end"]], 1).astype(np.float64)[perm]
    gt_offsets = np.concatenate([[0], np.cumsum(np.bincount(gt_key, minlength=G))]).astype(np.int32)
    npos = np.bincount(gt_cls, minlength=C).astype(np.int32)

    cls, keep = remap(np.asarray(preds["label"]), gt_labels)
    vid = np.array([number.get(v, len(number)) for v in preds["video-id"]], np.int64)[keep]
    cls = cls[keep]
    seg = np.stack([preds["t-start"], preds["t-end"]], 1).astype(np.float64)[keep]
    score = np.asarray(preds["score"], np.float64)[keep]
    n = len(score)
    by_score = np.argsort(-score, kind="stable")
    key = (vid * C + cls)[by_score]
    grouped = np.argsort(key, kind="stable")
    pred_seg = seg[by_score[grouped]]
    pred_offsets = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=G))]).astype(np.int32)
    match = match_groups(pred_seg, pred_offsets, gt_seg, gt_offsets, thresholds, margins)
    by_class = np.argsort(cls[by_score], kind="stable")
    where = np.empty(n, np.int64)
    where[grouped] = np.arange(n)
    order = where[by_class].astype(np.int32)
    class_offsets = np.concatenate([[0], np.cumsum(np.bincount(cls, minlength=C))]).astype(np.int32)
    ap = np.zeros((len(thresholds), C))
    for c in range(C):
        rows = order[class_offsets[c]:class_offsets[c + 1]]
        if len(rows):
            ap[:, c] = ap_from_tp(match[:, rows] >= 0, npos[c])
    return dict(pred_seg=pred_seg, pred_offsets=pred_offsets, gt_seg=gt_seg, gt_offsets=gt_offsets, match=match, order=order,
                class_offsets=class_offsets, npos=npos, ap=ap)


def postprocess(results, cls_scores, num_pred, topk):
    """``postprocess_results``: dict of columns (``video-id`` a list; the rest numpy)."""
    vids = sorted(set(results["video-id"]))
    ids = np.asarray(results["video-id"], dtype=object)
    out = {"video-id": [], "t-start": [], "t-end": [], "label": [], "score": []}
    for v in vids:
        rows = np.where(ids == v)[0]
        score = np.asarray(results["score"], np.float64)[rows]
        rows = rows[np.argsort(-score, kind="stable")[:num_pred]]
        score = np.asarray(results["score"], np.float64)[rows]
        cs = np.asarray(cls_scores[v], np.float64)
        top = np.argsort(-cs, kind="stable")[:topk]
        out["video-id"] += [v] * (len(rows) * topk)
        out["score"].append(np.sqrt(cs[top][:, None] * score[None, :]).flatten())
        out["t-start"].append(np.tile(np.asarray(results["t-start"], np.float64)[rows], topk))
        out["t-end"].append(np.tile(np.asarray(results["t-end"], np.float64)[rows], topk))
        out["label"].append(np.repeat(top, len(rows)))
    for k in ("t-start", "t-end", "label", "score"):
        out[k] = np.concatenate(out[k])
    return out
