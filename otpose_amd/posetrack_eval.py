"""PoseTrack / poseval pose AP on the GPU: the number the reference reports after every validation epoch and picks its best
checkpoint by (script/Common.py:442 -> dataset/PoseTrackDataset.py:453-608 ``evaluate`` -> utils/evaluate.py ``evaluate_ap``).

``pack_ground_truth`` walks the poseval-format annotation dicts once per dataset; ``PoseTrackEvaluator`` collects the device
tensors ``OTPose.predict`` returns and evaluates them with two kernels (``ops.pose_assign``, ``ops.ap_curve``; csrc/poseval.hip).
With a ``PoseNMS`` the evaluator first rescores the persons and suppresses duplicate poses per frame by OKS, hard or soft
(``ops.pose_nms``; csrc/posenms.hip) - the post-processing of predictions made on detector boxes.
Out of scope: MOTA / tracking, the JSON directory layout of poseval, YOLO boxes, image dumps.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

from . import ops

NUM_JOINTS = ops.POSEVAL_JOINTS
MAX_PR = ops.POSEVAL_MAX_PR
MAX_GT = ops.POSEVAL_MAX_GT
# coco2posetrack_ord (utils/keypoints.py:7-28): official joint k <- index in the model's 17-joint ordering
COCO_OF_OFFICIAL = (16, 14, 12, 11, 13, 15, 10, 8, 6, 5, 7, 9, 1, 0, 2)
TABLE_KEYS = ("Head", "Shoulder", "Elbow", "Wrist", "Hip", "Knee", "Ankle", "Mean")
_GT_KEYS = ("gt_off", "gt_xy", "gt_has", "gt_head", "poly_off", "vert_off", "vert_xy")


def _rect_has_points(rect):
    """rectHasPoints (utils/evaluate.py:70-73)."""
    return ("annopoints" in rect and len(rect["annopoints"]) > 0 and len(rect["annopoints"][0]) > 0
            and "point" in rect["annopoints"][0])


def pack_ground_truth(annolist_frames):
    """poseval-format frames (``annorect`` -> ``annopoints[0].point`` with ``id/x/y``, ``x1..y2``; optional
    ``ignore_regions`` -> ``point`` with ``x/y``) -> the packed arrays of ``ops.pose_assign`` (numpy) plus ``kept``, the
    indices of the frames that stay, ``frame_map`` (original index -> packed index or -1) and ``num_frames``.

    cleanupData (utils/evaluate.py:85-99): a frame whose ``annorect`` is empty is dropped (and with it its predictions), a
    rect without points is dropped.  A rect whose point list is empty stays (a person with no annotated joint).  Raises
    ``ValueError`` for a joint id outside [0, 15), a joint given twice, a polygon with fewer than 3 vertices or more than
    ``MAX_GT`` persons in a frame."""
    kept, gt_off, poly_off, vert_off = [], [0], [0], [0]
    xy, has, head, verts = [], [], [], []
    for fi, frame in enumerate(annolist_frames):
        if len(frame["annorect"]) == 0:
            continue
        kept.append(fi)
        n = 0
        for rect in frame["annorect"]:
            if not _rect_has_points(rect):
                continue
            p = np.zeros((NUM_JOINTS, 2), np.float64)
            m = 0
            for pt in rect["annopoints"][0]["point"]:
                k = int(pt["id"][0])
                if not 0 <= k < NUM_JOINTS:
                    raise ValueError(f"frame {fi}: joint id {k} outside [0, {NUM_JOINTS})")
                if m >> k & 1:
                    raise ValueError(f"frame {fi}: joint id {k} given twice")
                m |= 1 << k
                p[k] = (float(pt["x"][0]), float(pt["y"][0]))
            xy.append(p)
            has.append(m)
            head.append([float(rect[c][0]) for c in ("x1", "y1", "x2", "y2")])
            n += 1
        if n > MAX_GT:
            raise ValueError(f"frame {fi} has {n} ground-truth persons, the kernel's limit is {MAX_GT}")
        gt_off.append(gt_off[-1] + n)
        for region in frame.get("ignore_regions", ()) or ():
            pts = region["point"]
            if len(pts) < 3:
                raise ValueError(f"frame {fi}: an ignore polygon with {len(pts)} vertices")
            verts.extend((float(q["x"][0]), float(q["y"][0])) for q in pts)
            vert_off.append(vert_off[-1] + len(pts))
        poly_off.append(len(vert_off) - 1)
    frame_map = np.full(len(annolist_frames), -1, np.int64)
    frame_map[np.asarray(kept, np.int64)] = np.arange(len(kept))
    return {
        "gt_off": np.asarray(gt_off, np.int32),
        "gt_xy": np.asarray(xy, np.float64).reshape(-1, NUM_JOINTS, 2),
        "gt_has": np.asarray(has, np.int32).reshape(-1),
        "gt_head": np.asarray(head, np.float64).reshape(-1, 4),
        "poly_off": np.asarray(poly_off, np.int32),
        "vert_off": np.asarray(vert_off, np.int32),
        "vert_xy": np.asarray(verts, np.float64).reshape(-1, 2),
        "kept": np.asarray(kept, np.int64),
        "frame_map": frame_map,
        "num_frames": len(annolist_frames),
    }


def pack_predictions(frame_map, frame_id, num_kept):
    """CSR of the predicted persons per kept frame: ``(pr_off (F+1) int32, pr_sample (NP) int32)``.  Samples of a dropped
    frame are left out, within a frame the samples keep their order of arrival (filenames_map, script/Common.py:413-416),
    and a frame without a sample gets the placeholder person -1 (convert_data_to_annorect_struct, utils/evaluate.py:787-796).
    Raises ``ValueError`` past ``MAX_PR`` persons in a frame."""
    frame_id = np.asarray(frame_id, np.int64).reshape(-1)
    packed = frame_map[frame_id] if frame_id.size else np.zeros(0, np.int64)
    sample = np.nonzero(packed >= 0)[0]
    sample = sample[np.argsort(packed[sample], kind="stable")]
    count = np.bincount(packed[sample], minlength=num_kept)
    if count.size and count.max() > MAX_PR:
        raise ValueError(f"kept frame {int(count.argmax())} has {int(count.max())} predicted persons, the kernel's limit "
                         f"is {MAX_PR}")
    slots = np.maximum(count, 1)
    pr_off = np.zeros(num_kept + 1, np.int64)
    np.cumsum(slots, out=pr_off[1:])
    pr_sample = np.full(int(pr_off[-1]), -1, np.int64)
    start = np.repeat(pr_off[:-1][count > 0], count[count > 0])
    first = np.repeat(np.cumsum(count)[count > 0] - count[count > 0], count[count > 0])
    pr_sample[start + np.arange(sample.size) - first] = sample
    return pr_off.astype(np.int32), pr_sample.astype(np.int32)


def cum_table(ap):
    """getCum (utils/evaluate.py:136-150) of the 16 values as the ``name_value`` of PoseTrackDataset.evaluate (:595-606)."""
    v = np.asarray(ap, np.float64).reshape(16)
    cum = [v[[14, 12, 13]].mean(), v[[8, 9]].mean(), v[[7, 10]].mean(), v[[6, 11]].mean(), v[[2, 3]].mean(),
           v[[1, 4]].mean(), v[[0, 5]].mean(), v[15]]
    return OrderedDict(zip(TABLE_KEYS, (float(c) for c in cum)))


def with_mean(per_joint):
    """compute_metrics' closing row (utils/evaluate.py:724-729): the mean over the joints that are not NaN."""
    v = np.asarray(per_joint, np.float64).reshape(NUM_JOINTS)
    return np.concatenate([v, [v[~np.isnan(v)].mean()]])


class PoseNMS:
    """Settings of the pose NMS (``ops.pose_nms``): ``oks_thresh`` (OKS_THRE), ``in_vis_thre`` (IN_VIS_THRE: the joints that
    count in a person's score), ``soft`` (SOFT_NMS) with ``soft_type`` "gaussian" / "linear" and ``max_dets``,
    ``oks_in_vis_thre`` (the joint selection inside the OKS; None as HRNet calls it) and the per-joint ``sigmas``."""

    def __init__(self, oks_thresh=0.9, in_vis_thre=0.0, soft=False, soft_type="gaussian", max_dets=20,
                 oks_in_vis_thre=None, sigmas=ops.COCO_SIGMAS):
        self.oks_thresh, self.in_vis_thre, self.soft = float(oks_thresh), float(in_vis_thre), bool(soft)
        self.soft_type, self.max_dets, self.oks_in_vis_thre = soft_type, int(max_dets), oks_in_vis_thre
        self.sigmas = tuple(float(s) for s in sigmas)

    @classmethod
    def from_cfg(cls, cfg, phase):
        """The settings of ``cfg.VAL`` (``phase`` "validate", as dataset/PoseTrackDataset.py:57 spells it, or "val") or
        ``cfg.TEST`` (any other phase): IN_VIS_THRE, OKS_THRE, SOFT_NMS (configs/default.py:168-195).  ``None`` - no NMS -
        when POST_PROCESS is false or absent.  NMS_THRE is not read."""
        node = cfg.get("VAL" if str(phase).lower() in ("validate", "val") else "TEST") or {}
        if not node.get("POST_PROCESS", False):
            return None
        return cls(oks_thresh=node.get("OKS_THRE", 0.5), in_vis_thre=node.get("IN_VIS_THRE", 0.0),
                       soft=node.get("SOFT_NMS", False))

    def kwargs(self):
        return {"oks_thresh": self.oks_thresh, "in_vis_thre": self.in_vis_thre, "oks_in_vis_thre": self.oks_in_vis_thre,
                "sigmas": self.sigmas, "soft": self.soft, "soft_type": self.soft_type, "max_dets": self.max_dets}


class PoseTrackEvaluator:
    """Collects predictions on the device and evaluates the PoseTrack AP table against a packed ground truth.

    ``gt`` is :func:`pack_ground_truth`'s result (or the annotation frames themselves).  ``add`` appends device tensors; no
    prediction is copied to the host before ``summarize`` has reduced them to 15 x 3 numbers.  ``nms`` (a :class:`PoseNMS`
    or None) suppresses duplicate poses per frame before the assignment; ``add`` then needs each sample's box area."""

    def __init__(self, gt, dist_thresh=0.5, nms=None):
        self.gt = gt if isinstance(gt, dict) else pack_ground_truth(gt)
        self.dist_thresh = float(dist_thresh)
        self.nms = nms
        self._gt_dev = None
        self.reset()

    def reset(self):
        self._preds, self._maxvals, self._box, self._frame, self._area = [], [], [], [], []

    def add(self, preds, maxvals, box_score, frame_id, area=None, scale=None):
        """``preds`` (B,17,2) / ``maxvals`` (B,17,1) float32 as ``OTPose.predict`` / ``ops.get_final_preds`` return them,
        ``box_score`` (B,) the detector's box score per sample (kept in float64), ``frame_id`` (B,) the index of each
        sample's frame in the ORIGINAL ground-truth frame list.  Samples of a dropped frame are ignored.  With ``nms`` set,
        ``area`` (B,) is each sample's box area, or ``scale`` (B,2) the crop's scale, from which the area is formed in
        float64 as ``prod(scale * 200)`` (``all_boxes[:, 4]``, script/Common.py:429)."""
        if not torch.is_tensor(preds) or not torch.is_tensor(maxvals):
            raise TypeError("preds and maxvals must be tensors")
        b = preds.shape[0]
        if preds.dtype != torch.float32 or maxvals.dtype != torch.float32 or tuple(preds.shape) != (b, 17, 2) \
                or maxvals.numel() != b * 17:
            raise ValueError("preds must be (B,17,2) float32 and maxvals (B,17,1) float32")
        if torch.is_tensor(frame_id):
            frame_id = frame_id.detach().cpu().numpy()
        frame_id = np.asarray(frame_id).reshape(-1).astype(np.int64)
        box = torch.as_tensor(box_score, dtype=torch.float64).reshape(-1)
        if frame_id.size != b or box.numel() != b:
            raise ValueError("box_score and frame_id must have one entry per sample")
        if b and (frame_id.min() < 0 or frame_id.max() >= self.gt["num_frames"]):
            raise ValueError(f"frame_id outside [0, {self.gt['num_frames']})")
        if self.nms is not None:
            if area is None and scale is None:
                raise ValueError("the evaluator has an NMS: add() needs area= or scale=")
            if area is None:
                area = (torch.as_tensor(scale, dtype=torch.float64).reshape(-1, 2) * 200.0).prod(1)
            area = torch.as_tensor(area, dtype=torch.float64).reshape(-1)
            if area.numel() != b:
                raise ValueError("area / scale must have one entry per sample")
            self._area.append(area.to(preds.device))
        self._preds.append(preds.detach().reshape(b, 17, 2))
        self._maxvals.append(maxvals.detach().reshape(b, 17, 1))
        self._box.append(box.to(preds.device))
        self._frame.append(frame_id)

    def _gathered(self):
        if not self._preds:
            raise RuntimeError("no predictions were added")
        frame_id = np.concatenate(self._frame)
        return torch.cat(self._preds), torch.cat(self._maxvals), torch.cat(self._box), frame_id

    def _survivors(self, pr_off, pr_sample, preds, maxvals, box):
        """The CSR (device tensors) after ``ops.pose_nms``: the survivors of each frame in their order of arrival.  Every
        frame keeps at least the head of its order (or its placeholder), so no frame becomes empty."""
        dev = preds.device
        off, sample = torch.from_numpy(pr_off).to(dev), torch.from_numpy(pr_sample).to(dev)
        keep = ops.pose_nms(off, sample, preds, maxvals, box, torch.cat(self._area), **self.nms.kwargs())[0]
        before = torch.zeros(keep.numel() + 1, dtype=torch.int32, device=dev)
        before[1:] = keep.cumsum(0)
        return before[off.long()].contiguous(), sample[keep]

    def kept_samples(self):
        """Indices (ascending, numpy int64) of the added samples that reach the assignment: those of a kept frame and,
        with ``nms``, not suppressed."""
        preds, maxvals, box, frame_id = self._gathered()
        g = self.gt
        pr_off, pr_sample = pack_predictions(g["frame_map"], frame_id, len(g["kept"]))
        if self.nms is not None:
            pr_sample = self._survivors(pr_off, pr_sample, preds, maxvals, box)[1].cpu().numpy()
        return np.sort(pr_sample[pr_sample >= 0].astype(np.int64))

    def assign(self):
        """``ops.pose_assign`` over everything added: ``(labels, scores, ngt, pr_off, pr_sample)`` (the last two numpy);
        with ``nms`` over the survivors of ``ops.pose_nms``, the CSR returned being theirs."""
        preds, maxvals, box, frame_id = self._gathered()
        g = self.gt
        pr_off, pr_sample = pack_predictions(g["frame_map"], frame_id, len(g["kept"]))
        dev = preds.device
        if self.nms is not None:
            off_dev, sample_dev = self._survivors(pr_off, pr_sample, preds, maxvals, box)
            pr_off, pr_sample = off_dev.cpu().numpy(), sample_dev.cpu().numpy()
        else:
            off_dev, sample_dev = torch.from_numpy(pr_off).to(dev), torch.from_numpy(pr_sample).to(dev)
        if self._gt_dev is None or self._gt_dev[0] != dev:
            self._gt_dev = (dev, {k: torch.from_numpy(g[k]).to(dev) for k in _GT_KEYS})
        d = self._gt_dev[1]
        labels, scores, ngt = ops.pose_assign(
            off_dev, sample_dev, preds, maxvals, box, d["gt_off"],
            d["gt_xy"], d["gt_has"], d["gt_head"], d["poly_off"], d["vert_off"], d["vert_xy"], self.dist_thresh)
        return labels, scores, ngt, pr_off, pr_sample

    def summarize(self):
        """``{"ap", "precision", "recall": (16,) float64 numpy, "table": OrderedDict}``: apAll / preAll / recAll of
        compute_metrics (15 joints + their mean) and the ``name_value`` of PoseTrackDataset.evaluate;
        ``table["Mean"]`` is the reference's ``perf_indicator``.  Entries of equal score are ordered as
        ``ops.sort_entries`` states (the reference's own order of ties is that of an unstable sort)."""
        labels, scores, ngt, _, _ = self.assign()
        lab, joint_off, _ = ops.sort_entries(labels, scores)
        out = ops.ap_curve(lab, joint_off, ngt.sum(0, dtype=torch.int64)).cpu().numpy()
        ap, pre, rec = (with_mean(out[:, c]) for c in range(3))
        return {"ap": ap, "precision": pre, "recall": rec, "table": cum_table(ap)}

    def annolist(self):
        """The prediction frames as the reference writes them for poseval (PoseTrackDataset.py:573-577 with
        convert_data_to_annorect_struct and coco2posetrack_ord): one ``{"annorect": [...]}`` per ORIGINAL ground-truth frame,
        official joint order, score = float64(maxval) * box score, the placeholder person where nothing was predicted.
        With ``nms`` only the persons it keeps are written (a dropped frame, which is not evaluated, keeps all of its samples).  This copies the predictions to the host."""
        preds, maxvals, box, frame_id = self._gathered()
        kept = None if self.nms is None else set(self.kept_samples().tolist())
        preds = preds.cpu().numpy().astype(np.float64)
        maxvals = maxvals.cpu().numpy().reshape(-1, 17).astype(np.float64)
        box = box.cpu().numpy()
        per_frame = [[] for _ in range(self.gt["num_frames"])]
        for s, f in enumerate(frame_id):
            if kept is None or s in kept or self.gt["frame_map"][f] < 0:
                per_frame[f].append(s)
        frames = []
        for samples in per_frame:
            rects = []
            for track, s in enumerate(samples):
                g = float(box[s])
                point = [{"id": [k], "x": [float(preds[s, c, 0])], "y": [float(preds[s, c, 1])],
                          "score": [float((maxvals[s, c] + maxvals[s, c]) / 2.0 * g)]}
                         for k, c in enumerate(COCO_OF_OFFICIAL)]
                rects.append({"annopoints": [{"point": point}], "score": [g], "track_id": [track]})
            if not samples:
                rects.append({"annopoints": [{"point": [{"id": [0], "x": [0], "y": [0], "score": [-100.0]}]}],
                              "score": [0], "track_id": [0]})
            frames.append({"annorect": rects})
        return frames
