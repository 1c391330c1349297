"""Float32 restatement of the reference's temporal segment NMS: the two C++ loops of thirdparty/utils/csrc/nms_cpu.cpp
(``nms_1d``, ``softnms_1d``) and the Python layer of thirdparty/utils/nms.py (``NMSop_apply``, ``SoftNMSop_apply``,
``seg_voting``, ``batched_nms``), in numpy.  tests/golden/make_golden_segnms.py asserts that the two loops reproduce the
built extension bit for bit on every recorded case.

Every value is float32 and every operation is rounded on its own, as in the scalar C++.  The arithmetic of a round is
written over arrays - within a round every segment meets the taken one exactly once, whatever the order - and the
reference's array permutation (swap the arg-max to position i, swap a dropped segment with the last) is replayed position by
position, so that ``inds`` and the tie order of its first-maximum scan are the reference's.  ``exp`` is the C library's
``expf``, which ``std::exp(float)`` calls.

``margins``: a dict that receives the smallest distance of every discrete decision from its threshold:
``top2`` (relative gap of the two highest live scores at a selection), ``ovr`` (|ovr - iou_threshold| of every tested
overlap), ``min_score`` (relative distance of every tested score from a positive ``min_score``), ``distinct`` (smallest gap of
the input scores), ``vote`` (|iou - voting threshold|), ``final`` (relative gap of neighbours in batched_nms's last sort).
"""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]


def _expf(a):
    return np.array([_libm.expf(v) for v in a.tolist()], F)


def _note(margins, key, value):
    if margins is not None and value == value:
        margins[key] = min(margins.get(key, np.inf), float(value))


def _areas(segs):
    x1, x2 = segs[:, 0].astype(F), segs[:, 1].astype(F)
    return x1.copy(), x2.copy(), (x2 - x1) + F(1e-6)


def _ovr(ix1, ix2, iarea, x1, x2, areas):
    inter = np.maximum(F(0), np.minimum(ix2, x2) - np.maximum(ix1, x1))
    return inter / (iarea + areas - inter)


def _note_distinct(margins, scores):
    if margins is not None and len(scores) > 1:
        _note(margins, "distinct", np.diff(np.sort(scores.astype(np.float64))).min())


def nms_1d(segs, scores, iou_threshold, margins=None):
    """nms_cpu.cpp:19-58 -> int64 indices of the kept segments in descending-score order."""
    n = segs.shape[0]
    if segs.size == 0:
        return np.zeros(0, np.int64)
    thr = F(iou_threshold)
    x1, x2, areas = _areas(segs)
    _note_distinct(margins, scores)
    order = np.argsort(-scores.astype(F), kind="stable")
    select = np.ones(n, bool)
    for _i in range(n):
        if not select[_i]:
            continue
        i, js = order[_i], order[_i + 1:]
        ovr = _ovr(x1[i], x2[i], areas[i], x1[js], x2[js], areas[js])
        live = select[_i + 1:]
        if live.any():
            _note(margins, "ovr", np.abs(ovr[live].astype(np.float64) - float(thr)).min())
        select[_i + 1:] = live & ~(ovr >= thr)
    return order[select].astype(np.int64)


def softnms_1d(segs, scores, iou_threshold, sigma, min_score, method, margins=None):
    """nms_cpu.cpp:67-160 -> (dets (n, 3) float32 with the first len(inds) rows written, inds int64)."""
    n = segs.shape[0]
    dets = np.zeros((n, 3), F)
    if segs.size == 0:
        return dets, np.zeros(0, np.int64)
    thr, sig, ms = F(iou_threshold), F(sigma), F(min_score)
    x1, x2, areas = _areas(segs)
    sc = scores.astype(F).copy()
    inds = np.arange(n, dtype=np.int64)
    _note_distinct(margins, scores)
    nsegs, i = n, 0
    while i < nsegs:
        live = sc[i:nsegs]
        max_pos = i + int(np.argmax(live))                        # the first maximum: `max_score < sc[pos]` is strict
        if margins is not None and nsegs - i > 1:
            top = np.sort(live.astype(np.float64))[-2:]
            _note(margins, "top2", (top[1] - top[0]) / abs(top[1]) if top[1] != 0 else 0.0)
        ix1, ix2, iscore, iarea, iind = x1[max_pos], x2[max_pos], sc[max_pos], areas[max_pos], inds[max_pos]
        dets[i] = (ix1, ix2, iscore)
        for a, v in ((x1, ix1), (x2, ix2), (sc, iscore), (areas, iarea), (inds, iind)):
            a[max_pos] = a[i]
            a[i] = v
        lo = i + 1
        if lo < nsegs:
            ovr = _ovr(ix1, ix2, iarea, x1[lo:nsegs], x2[lo:nsegs], areas[lo:nsegs])
            weight = np.ones(nsegs - lo, F)
            if method == 0:
                weight[ovr >= thr] = F(0)
            elif method == 1:
                weight = np.where(ovr >= thr, F(1) - ovr, F(1)).astype(F)
            elif method == 2:
                weight = _expf(-(ovr * ovr) / sig)
            if method in (0, 1):
                _note(margins, "ovr", np.abs(ovr.astype(np.float64) - float(thr)).min())
            sc[lo:nsegs] = sc[lo:nsegs] * weight
            if ms > 0:
                _note(margins, "min_score", (np.abs(sc[lo:nsegs].astype(np.float64) - float(ms)) / float(ms)).min())
            drop = (sc[lo:nsegs] < ms).tolist()
            if any(drop):                                         # the swap-with-last of lines 146-154, position by position
                drop = [False] * lo + drop
                pos = lo
                while pos < nsegs:
                    if drop[pos]:
                        last = nsegs - 1
                        for a in (x1, x2, sc, areas, inds):
                            a[pos] = a[last]
                        drop[pos] = drop[last]
                        nsegs -= 1
                    else:
                        pos += 1
        i += 1
    return dets, inds[:nsegs].copy()


def NMSop_apply(segs, cls_idxs, scores, iou_threshold, min_score, max_num, margins=None):
    """nms.py:8-35."""
    if min_score > 0:
        valid = scores > F(min_score)
        _note(margins, "min_score", (np.abs(scores.astype(np.float64) - float(F(min_score))) / float(F(min_score))).min()
              if len(scores) else np.inf)
        segs, scores, cls_idxs = segs[valid], scores[valid], cls_idxs[valid]
    inds = nms_1d(segs, scores, iou_threshold, margins)
    if max_num > 0:
        inds = inds[:min(max_num, len(inds))]
    return segs[inds].copy(), scores[inds].copy(), cls_idxs[inds].copy()


def SoftNMSop_apply(segs, scores, cls_idxs, iou_threshold, sigma, min_score, method, max_num, margins=None):
    """nms.py:38-64."""
    dets, inds = softnms_1d(segs, scores, iou_threshold, sigma, min_score, method, margins)
    n_segs = min(len(inds), max_num) if max_num > 0 else len(inds)
    return dets[:n_segs, :2].copy(), dets[:n_segs, 2].copy(), cls_idxs[inds][:n_segs].copy()


def seg_voting(nms_segs, all_segs, all_scores, iou_threshold, score_offset=1.5, margins=None):
    """nms.py:67-101 (the offset scores are computed and unused there; the weights are the raw scores)."""
    a, b = nms_segs.astype(F)[:, None, :], all_segs.astype(F)[None, :, :]
    inter = np.maximum(np.minimum(a[..., 1], b[..., 1]) - np.maximum(a[..., 0], b[..., 0]), F(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / ((a[..., 1] - a[..., 0]) + (b[..., 1] - b[..., 0]) - inter)
        if iou.size:
            _note(margins, "vote", np.nanmin(np.abs(iou.astype(np.float64) - float(F(iou_threshold)))))
        w = (iou >= F(iou_threshold)).astype(F) * all_scores.astype(F)[None, :]
        w = w / w.sum(axis=1, keepdims=True, dtype=F)
        return (w @ all_segs.astype(F)).astype(F)


def batched_nms(segs, scores, cls_idxs, iou_threshold, min_score, max_seg_num, use_soft_nms=True, multiclass=True, sigma=0.5,
                voting_thresh=0.75, margins=None):
    """nms.py:104-191."""
    if segs.shape[0] == 0:
        return np.zeros((0, 2), F), np.zeros(0, F), np.zeros(0, cls_idxs.dtype)

    def one(s, p, c):
        if use_soft_nms:
            return SoftNMSop_apply(s, p, c, iou_threshold, sigma, min_score, 2, max_seg_num, margins)
        return NMSop_apply(s, c, p, iou_threshold, min_score, max_seg_num, margins)

    if multiclass:
        parts = [one(segs[cls_idxs == c], scores[cls_idxs == c], cls_idxs[cls_idxs == c]) for c in np.unique(cls_idxs)]
        new_segs, new_scores, new_cls = (np.concatenate([p[k] for p in parts]) for k in range(3))
    else:
        new_segs, new_scores, new_cls = one(segs, scores, cls_idxs)
        if voting_thresh > 0:
            new_segs = seg_voting(new_segs, segs, scores, voting_thresh, margins=margins)
    idxs = np.argsort(-new_scores, kind="stable")
    if margins is not None and len(idxs) > 1:
        s = new_scores[idxs].astype(np.float64)
        _note(margins, "final", ((s[:-1] - s[1:]) / np.abs(s[:-1])).min())
    idxs = idxs[:min(max_seg_num, new_segs.shape[0])]
    return new_segs[idxs], new_scores[idxs], new_cls[idxs]
