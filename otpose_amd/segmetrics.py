"""Temporal detection mAP on the GPU: the names and call signatures of the reference's ``thirdparty/utils/metrics.py``
(``ANETdetection``, ``compute_average_precision_detection``, ``load_gt_seg_from_json``, ``load_pred_seg_from_json``) and of
``thirdparty/utils/postprocessing.py`` (``postprocess_results``, ``results_to_dict``, ``results_to_array``) over the kernels of
csrc/segap.hip.  Neither pandas nor joblib is imported; a table is a dict of columns (or anything indexable by column name,
a pandas DataFrame included).

Every (video, class) pair is one group, as in segnms.py: the predictions are sorted by score and by group on the device, the
offsets come from the group sizes, ``ops.seg_ap_match`` assigns predictions to ground truths for every group and threshold in
one launch, one more sort gives the per-class score order, and ``ops.seg_ap`` turns the matches into interpolated AP.  JSON
files are parsed and video ids are turned into integers on the host (a dict lookup per row); segments, scores and labels
stay where they are.  DESIGN.md section 3.15.

One deviation: the reference remaps prediction labels with ``DataFrame.replace(activity_index)``, which leaves a label that
is absent from the ground truth unchanged, so it can collide with a remapped index and be scored as another class.  Here such
predictions are dropped, which is what the comment at metrics.py:117 intends.
"""
from __future__ import annotations

import json
import os
import pickle

import numpy as np
import torch

from . import ops

__all__ = ["ANETdetection", "compute_average_precision_detection", "load_gt_seg_from_json", "load_pred_seg_from_json",
           "remap_labels", "postprocess_results", "results_to_dict", "results_to_array"]


# ---- host side: files and tables -------------------------------------------------------------------------------------------
def _label_id(value, label_offset):
    """A label entry of the JSON: an integer, or a list folded as metrics.py:32-39 folds it."""
    if isinstance(value, (tuple, list)):
        return sum(label_offset ** i + int(x) for i, x in enumerate(reversed(value)))
    return int(value)


def _database(json_file):
    with open(json_file, "r", encoding="utf8") as f:
        return json.load(f)["database"]


def _table(vids, starts, stops, labels, scores=None):
    out = {"video-id": np.array(vids, dtype=object), "t-start": np.array(starts, np.float64),
           "t-end": np.array(stops, np.float64), "label": np.array(labels, np.int64)}
    if scores is not None:
        out["score"] = np.array(scores, np.float64)
    return out


def load_gt_seg_from_json(json_file, split=None, label="label_id", label_offset=0):
    """metrics.py:13-50 as a dict of numpy columns ``video-id`` (object), ``t-start``, ``t-end`` (float64), ``label`` (int64):
    the annotations of every video of the database whose ``subset`` is ``split`` (all of them when ``split`` is None)."""
    vids, starts, stops, labels = [], [], [], []
    for vid, entry in _database(json_file).items():
        if split is not None and entry["subset"].lower() != split:
            continue
        for event in entry["annotations"]:
            vids.append(vid)
            starts.append(float(event["segment"][0]))
            stops.append(float(event["segment"][1]))
            labels.append(_label_id(event[label], label_offset))
    return _table(vids, starts, stops, labels)


def load_pred_seg_from_json(json_file, label="label_id", label_offset=0):
    """metrics.py:53-87 as a dict of numpy columns: the gt columns and ``score`` (float64, the entries' ``scores`` field)."""
    vids, starts, stops, labels, scores = [], [], [], [], []
    for vid, events in _database(json_file).items():
        for event in events:
            vids.append(vid)
            starts.append(float(event["segment"][0]))
            stops.append(float(event["segment"][1]))
            labels.append(_label_id(event[label], label_offset))
            scores.append(float(event["scores"]))
    return _table(vids, starts, stops, labels, scores)


def _ids(column):
    """A ``video-id`` column as a host list."""
    if torch.is_tensor(column):
        return column.tolist()
    if isinstance(column, np.ndarray):
        return column.tolist()
    return list(column)


def _dev(column, dtype, device):
    """A numeric column as a 1-D tensor of ``dtype`` on ``device``; widening float32 to float64 is exact."""
    if not torch.is_tensor(column):
        column = torch.from_numpy(np.ascontiguousarray(np.asarray(column)))
    return column.detach().reshape(-1).to(device=device, dtype=dtype)


def _host(column):
    return column.detach().cpu().numpy() if torch.is_tensor(column) else np.asarray(column)


def _offsets(lengths, device):
    off = torch.zeros(lengths.shape[0] + 1, dtype=torch.int32, device=device)
    off[1:] = torch.cumsum(lengths, 0)
    return off


def remap_labels(labels, gt_labels):
    """``(index, keep)`` of ``labels`` (N) against the sorted distinct ground-truth labels ``gt_labels`` (C), both int64
    tensors on one device: ``index`` is the position of a label in ``gt_labels`` (the reference's ``activity_index``) and
    ``keep`` is False for a label that is not among them (such predictions are dropped, see the module docstring)."""
    index = torch.searchsorted(gt_labels, labels).clamp_(max=gt_labels.shape[0] - 1)
    return index, gt_labels[index] == labels


# ---- the ground truth, grouped once ----------------------------------------------------------------------------------------
class _GroundTruth:
    """Ground-truth segments sorted by (video, class) group.  ``video_index``: host dict video id -> 0 .. V-1; group
    ``v * C + c``; the video number V stands for every video without ground truth, so there are (V + 1) C groups."""

    def __init__(self, video_ids, seg, cls, n_classes, device):
        self.video_index = {}
        for v in video_ids:
            self.video_index.setdefault(v, len(self.video_index))
        self.n_classes, self.device = n_classes, device
        self.n_groups = (len(self.video_index) + 1) * n_classes
        if self.n_groups >= 2 ** 31 or seg.shape[0] >= 2 ** 28:
            raise ValueError("too many (video, class) groups or ground-truth segments for 32-bit offsets")
        vid = torch.tensor([self.video_index[v] for v in video_ids], dtype=torch.int64, device=device)
        key, perm = torch.sort(vid * n_classes + cls, stable=True)
        self.seg = seg[perm].contiguous()
        self.offsets = _offsets(torch.bincount(key, minlength=self.n_groups), device)
        self.npos = torch.bincount(cls, minlength=n_classes).to(torch.int32)

    def videos(self, video_ids):
        """The video number of every row of a prediction table."""
        index, other = self.video_index, len(self.video_index)
        return torch.tensor([index.get(v, other) for v in video_ids], dtype=torch.int64, device=self.device)


def _detection_ap(gt, vid, seg, cls, score, thresholds):
    """``ap`` (T, C) float64 on the device for predictions ``vid`` / ``cls`` (N) int64, ``seg`` (N, 2) and ``score`` (N)
    float64 against the grouped ground truth ``gt``.  Exactly equal scores are ordered by input row."""
    n, c, dev = seg.shape[0], gt.n_classes, gt.device
    if n == 0:
        return torch.zeros((len(thresholds), c), dtype=torch.float64, device=dev)
    if n >= 2 ** 28:
        raise ValueError("too many predictions for 32-bit offsets")
    by_score = torch.sort(score, descending=True, stable=True)[1]
    cls_s = cls[by_score]
    # group order: a stable sort by group over the score order leaves every group in descending score
    key, grouped = torch.sort(vid[by_score] * c + cls_s, stable=True)
    pred_offsets = _offsets(torch.bincount(key, minlength=gt.n_groups), dev)
    match = ops.seg_ap_match(seg[by_score[grouped]].contiguous(), pred_offsets, gt.seg, gt.offsets, thresholds)
    # class-major score order, named by the rows of the grouped table
    cls_sorted, by_class = torch.sort(cls_s, stable=True)
    where = torch.empty(n, dtype=torch.int64, device=dev)
    where[grouped] = torch.arange(n, device=dev)
    class_offsets = _offsets(torch.bincount(cls_sorted, minlength=c), dev)
    return ops.seg_ap(match, where[by_class].to(torch.int32), class_offsets, gt.npos)


def _device_of(*columns):
    for col in columns:
        if torch.is_tensor(col) and col.is_cuda:
            return col.device
    return torch.device("cuda")


class ANETdetection(object):
    """metrics.py:90-199 on the GPU.  ``ant_file``: the annotation JSON (parsed on the host); or pass ``ground_truth=`` a
    table with the columns ``video-id``, ``t-start``, ``t-end``, ``label`` (``ant_file`` may then be None; ``split`` does not
    apply).  ``num_workers`` is accepted and unused.  The ground truth is grouped on ``device`` (default: the current GPU)
    in the constructor; labels are remapped to 0 .. C-1 by sorted ground-truth label (``activity_index``)."""

    def __init__(self, ant_file, split=None, tiou_thresholds=np.linspace(0.1, 0.5, 5), label="label_id", label_offset=0,
                 num_workers=8, dataset_name=None, *, ground_truth=None, device=None):
        self.tiou_thresholds = tiou_thresholds
        self.ap = None
        self.num_workers = num_workers
        self.split = split
        if dataset_name is not None:
            self.dataset_name = dataset_name
        else:
            self.dataset_name = os.path.basename(ant_file).replace(".json", "") if ant_file is not None else "ground_truth"
        if ground_truth is None:
            ground_truth = load_gt_seg_from_json(ant_file, split=split, label=label, label_offset=label_offset)
        video_ids = _ids(ground_truth["video-id"])
        if not video_ids:
            raise ValueError("the ground truth holds no segment")
        self.device = torch.device(device) if device is not None else _device_of(ground_truth["t-start"])
        labels = _dev(ground_truth["label"], torch.int64, self.device)
        self._gt_labels = torch.unique(labels)                                  # sorted
        self.activity_index = {int(j): i for i, j in enumerate(self._gt_labels.tolist())}
        cls, _ = remap_labels(labels, self._gt_labels)
        seg = torch.stack([_dev(ground_truth["t-start"], torch.float64, self.device),
                           _dev(ground_truth["t-end"], torch.float64, self.device)], 1)
        self._gt = _GroundTruth(video_ids, seg, cls, len(self.activity_index), self.device)
        self.ground_truth = {"video-id": np.array(video_ids, dtype=object), "t-start": _host(seg[:, 0]),
                             "t-end": _host(seg[:, 1]), "label": _host(cls)}

    def evaluate(self, preds, verbose=True):
        """metrics.py:153-199: ``preds`` is a table with the columns ``video-id``, ``t-start``, ``t-end``, ``label``,
        ``score`` (device tensors, CPU tensors or numpy arrays; a dict, a pandas DataFrame, ...) or the path of a JSON file.
        Returns ``(mAP (T,) numpy, average_mAP)`` and sets ``self.ap`` (T, C)."""
        if isinstance(preds, str):
            if not os.path.isfile(preds):
                raise FileNotFoundError(preds)
            preds = load_pred_seg_from_json(preds)
        self.ap = None
        dev = self.device
        label, keep = remap_labels(_dev(preds["label"], torch.int64, dev), self._gt_labels)
        vid = self._gt.videos(_ids(preds["video-id"]))
        seg = torch.stack([_dev(preds["t-start"], torch.float64, dev), _dev(preds["t-end"], torch.float64, dev)], 1)
        score = _dev(preds["score"], torch.float64, dev)
        if not (vid.shape[0] == seg.shape[0] == label.shape[0] == score.shape[0]):
            raise ValueError("the columns of preds differ in length")
        ap = _detection_ap(self._gt, vid[keep], seg[keep], label[keep], score[keep], self.tiou_thresholds)
        self.ap = ap.cpu().numpy()
        mAP = self.ap.mean(axis=1)
        average_mAP = mAP.mean()
        if verbose:
            print("[RESULTS] Action detection results on {:s}.".format(self.dataset_name))
            block = ""
            for tiou, tiou_mAP in zip(self.tiou_thresholds, mAP):
                block += "\n|tIoU = {:.2f}: mAP = {:.2f} (%)".format(tiou, tiou_mAP * 100)
            print(block)
            print("Avearge mAP: {:.2f} (%)".format(average_mAP * 100))
        return mAP, average_mAP


def compute_average_precision_detection(ground_truth, prediction, tiou_thresholds=np.linspace(0.1, 0.5, 5)):
    """metrics.py:202-282 for ONE class: ``ground_truth`` with the columns ``video-id``, ``t-start``, ``t-end`` and
    ``prediction`` with ``score`` besides.  Returns ``ap`` (T,) numpy float64.  An empty ground truth raises ``ValueError``
    (the reference divides by zero there); an empty prediction gives zeros."""
    gt_ids = _ids(ground_truth["video-id"])
    if not gt_ids:
        raise ValueError("compute_average_precision_detection: a class without ground truth has no average precision")
    pred_ids = _ids(prediction["video-id"]) if len(prediction) else []
    if not pred_ids:
        return np.zeros(len(tiou_thresholds))
    dev = _device_of(prediction["t-start"], prediction["score"], ground_truth["t-start"])
    seg = torch.stack([_dev(ground_truth["t-start"], torch.float64, dev), _dev(ground_truth["t-end"], torch.float64, dev)], 1)
    gt = _GroundTruth(gt_ids, seg, torch.zeros(len(gt_ids), dtype=torch.int64, device=dev), 1, dev)
    pseg = torch.stack([_dev(prediction["t-start"], torch.float64, dev), _dev(prediction["t-end"], torch.float64, dev)], 1)
    zeros = torch.zeros(len(pred_ids), dtype=torch.int64, device=dev)
    ap = _detection_ap(gt, gt.videos(pred_ids), pseg, zeros, _dev(prediction["score"], torch.float64, dev), tiou_thresholds)
    return ap[:, 0].cpu().numpy()


# ---- postprocessing.py -----------------------------------------------------------------------------------------------------
def _load(filename):
    if not os.path.isfile(filename):
        raise FileNotFoundError(filename)
    if ".json" in filename:
        with open(filename, "r") as f:
            loaded = json.load(f)
        return loaded["results"] if "results" in loaded else loaded              # ActivityNet's external scores
    with open(filename, "rb") as f:
        return pickle.load(f)


def _rows(results):
    return zip(_ids(results["video-id"]), _host(results["t-start"]).tolist(), _host(results["t-end"]).tolist(),
               _host(results["label"]).tolist(), _host(results["score"]).tolist())


def results_to_dict(results):
    """postprocessing.py:31-54: the result columns as the per-video lists a JSON file holds (host)."""
    out = {vid: [] for vid in sorted(set(_ids(results["video-id"])))}
    for vid, start, end, label, score in _rows(results):
        out[vid].append({"label": int(label), "score": float(score), "segment": [float(start), float(end)]})
    return out


def results_to_array(results, num_pred):
    """postprocessing.py:57-94: per video the ``num_pred`` highest-scoring rows as numpy arrays ``label``, ``score``,
    ``segment`` (host)."""
    lists = {vid: ([], [], []) for vid in sorted(set(_ids(results["video-id"])))}
    for vid, start, end, label, score in _rows(results):
        lists[vid][0].append(int(label))
        lists[vid][1].append(float(score))
        lists[vid][2].append([float(start), float(end)])
    out = {}
    for vid, (label, score, segment) in lists.items():
        label, score, segment = np.asarray(label), np.asarray(score), np.asarray(segment)
        inds = np.argsort(score)[::-1][:num_pred]
        out[vid] = {"label": label[inds], "score": score[inds], "segment": segment[inds]}
    return out


def postprocess_results(results, cls_score_file, num_pred=200, topk=2):
    """postprocessing.py:97-155 on the GPU: per video the ``num_pred`` highest-scoring segments are repeated for each of the
    ``topk`` highest external classification scores of the video, labelled with that class and scored
    ``sqrt(cls_score * score)`` in float64.  ``results``: a table (or the path of a pickled one); ``cls_score_file``: a JSON or
    pickle path, or a dict ``{video-id: scores}`` with one score list of the same length per video.  Returns the table with
    ``video-id`` as a host list and the other columns as device tensors (``t-start``, ``t-end``, ``score`` float64, ``label``
    int64), videos in sorted order, inside a video class-major and descending score.  Exactly equal scores keep their input
    order (the reference leaves them to ``argsort``)."""
    if isinstance(results, str):
        results = _load(results)
    cls_scores = _load(cls_score_file) if isinstance(cls_score_file, str) else cls_score_file
    ids = _ids(results["video-id"])
    vids = sorted(set(ids))
    dev = _device_of(results["score"], results["t-start"])
    if not vids:
        empty = torch.zeros(0, dtype=torch.float64, device=dev)
        return {"video-id": [], "t-start": empty, "t-end": empty.clone(), "label": empty.long(), "score": empty.clone()}
    number = {v: i for i, v in enumerate(vids)}
    table = torch.from_numpy(np.asarray([np.asarray(cls_scores[v], np.float64) for v in vids])).to(dev)
    if table.dim() != 2 or table.shape[1] < topk:
        raise ValueError("every video needs one list of at least topk classification scores, all of one length")
    vid = torch.tensor([number[v] for v in ids], dtype=torch.int64, device=dev)
    score = _dev(results["score"], torch.float64, dev)
    seg = torch.stack([_dev(results["t-start"], torch.float64, dev), _dev(results["t-end"], torch.float64, dev)], 1)

    # per video: descending score, cut at num_pred (a stable sort by video over the score order)
    by_score = torch.sort(score, descending=True, stable=True)[1]
    vid_sorted, by_video = torch.sort(vid[by_score], stable=True)
    rows = by_score[by_video]
    per_video = torch.bincount(vid, minlength=len(vids))
    start = torch.cumsum(per_video, 0) - per_video
    rows = rows[(torch.arange(rows.shape[0], device=dev) - start[vid_sorted]) < num_pred]
    kept = torch.clamp(per_video, max=num_pred)
    kept_start = torch.cumsum(kept, 0) - kept

    top_score, top_idx = torch.sort(table, dim=1, descending=True, stable=True)
    top_score, top_idx = top_score[:, :topk], top_idx[:, :topk]
    # output row -> (video, k, n): a video's block is topk runs of its kept rows
    out_video = torch.repeat_interleave(torch.arange(len(vids), device=dev), kept * topk)
    local = torch.arange(out_video.shape[0], device=dev) - (kept_start * topk)[out_video]
    k, n = torch.div(local, kept[out_video], rounding_mode="floor"), local % kept[out_video]
    src = rows[kept_start[out_video] + n]
    sizes = (kept * topk).tolist()
    return {"video-id": [v for v, size in zip(vids, sizes) for _ in range(size)],
            "t-start": seg[src, 0], "t-end": seg[src, 1], "label": top_idx[out_video, k],
            "score": torch.sqrt(top_score[out_video, k] * score[src])}
