"""Video -> keypoints without leaving the device: the detector's boxes become the crop plan in one launch
(``ops.pose_plan``), and the pose network runs at ONE fixed batch size, so its engine is built once.

The host recipe (INTEGRATION.md section 3b') copies the boxes to the host, computes ``crop.box_to_center_scale`` /
``crop.crop_matrix`` / ``crop.window`` there and calls ``OTPose.predict`` with however many persons the chunk holds - and
``predict`` rebuilds the engine (weights packed again, a new launch list, a new hipGraph) whenever that number changes.
:class:`VideoPose` reads one int32 back per call (the person count) and runs groups of ``capacity`` persons, the last one
padded with empty crops: padding costs compute, never a rebuild."""
from __future__ import annotations

import collections

import torch

from . import ops

VideoPoseResult = collections.namedtuple("VideoPoseResult", "preds maxvals box_score person_slot pr_off center scale")


class VideoPose:
    """``VideoPose(model, capacity)``: ``model`` an :class:`otpose_amd.OTPose` in eval mode on the GPU, ``capacity`` the
    number of persons per forward (the engine's batch; 2 x capacity clips under ``flip_test``).  ``flip_test`` /
    ``shift_heatmap`` as in ``OTPose.predict``; ``min_score``, ``enlarge``, ``posetrack18`` as in ``ops.pose_plan``."""

    def __init__(self, model, capacity, flip_test=False, shift_heatmap=False, min_score=0.0, enlarge=1.25, posetrack18=True):
        if isinstance(capacity, bool) or int(capacity) != capacity or int(capacity) < 1:
            raise ValueError(f"capacity must be a positive whole number, got {capacity!r}")
        if getattr(model, "window_frames", 5) != 5:
            raise ValueError("VideoPose needs a 5-frame model (crop.window has no other form)")
        if shift_heatmap and not flip_test:
            raise ValueError("shift_heatmap belongs to the flip test: pass flip_test=True")
        self.model = model
        self.capacity = int(capacity)
        self.flip_test = bool(flip_test)
        self.shift_heatmap = bool(shift_heatmap)
        self.min_score = float(min_score)
        self.enlarge = float(enlarge)
        self.posetrack18 = bool(posetrack18)

    def run(self, pool, boxes, scores, counts, frame_number, num_frames, detect=None, max_persons=None):
        """Keypoints of every person the detector found in the pool slots ``detect = (lo, hi)`` (default: all).

        ``pool`` (S, Hp, Wp, 3) uint8 RGB frames on the GPU; ``boxes`` / ``scores`` / ``counts`` as
        ``PersonDetector.detect(pool)`` returns them; ``frame_number`` / ``num_frames`` (S) int32 (host lists are uploaded)
        as for ``ops.pose_plan``.  ``max_persons`` bounds the rows of the plan (default: every box of the detect range, which
        cannot overflow); it is rounded up to a multiple of ``capacity``, and more persons than that raise ``ValueError``.

        Returns a :class:`VideoPoseResult` of device tensors in (frame, box) order: ``preds (total, 17, 2)`` in frame
        pixels, ``maxvals (total, 17, 1)``, ``box_score (total)`` float64, ``person_slot (total)`` int32, ``pr_off (S + 1)``
        int32, ``center`` / ``scale (total, 2)`` - the arguments of ``ops.pose_nms`` and ``PoseTrackEvaluator.add``
        (``pr_sample`` is ``arange(total)``, ``area`` is ``prod(scale * 200)``).  One host read: the person count."""
        model, cap = self.model, self.capacity
        if model.training:
            raise RuntimeError("VideoPose.run runs in eval mode (call model.eval())")
        if not torch.is_tensor(pool) or pool.dtype != torch.uint8 or pool.dim() != 4 or pool.shape[-1] != 3:
            raise TypeError("pool must be an (S, Hp, Wp, 3) uint8 tensor")
        s = pool.shape[0]
        dev = pool.device
        frame_number = _slots_i32(frame_number, dev)
        num_frames = _slots_i32(num_frames, dev)
        lo, hi = (0, s) if detect is None else (int(detect[0]), int(detect[1]))
        k = boxes.shape[1] if torch.is_tensor(boxes) and boxes.dim() == 3 else 0
        bound = max(0, hi - lo) * k if max_persons is None else int(max_persons)
        if bound < 0:
            raise ValueError("max_persons must not be negative")
        rows = max(1, -(-bound // cap)) * cap
        w_img, h_img = model.cfg.MODEL.IMAGE_SIZE
        plan = ops.pose_plan(boxes, scores, counts, frame_number, num_frames, image_size=(w_img, h_img), max_persons=rows,
                             detect=(lo, hi), min_score=self.min_score, enlarge=self.enlarge, posetrack18=self.posetrack18)
        if plan.pr_off.numel() != s + 1:
            raise ValueError(f"the detector output covers {plan.pr_off.numel() - 1} frames, the pool has {s}")
        total = int(plan.total)                                 # the call's one host read
        if total > rows:
            raise ValueError(f"the detector found {total} persons, the plan has room for {rows} (max_persons)")
        preds, maxvals = [], []
        for g in range(-(-total // cap)):
            r = slice(g * cap, (g + 1) * cap)
            if self.flip_test:
                x, mg = model.input_buffers(2 * cap, dev)
                ops.crop_clips(pool, plan.frame_idx[r], plan.M[r], out=x, mirror_pair=True)
                _, p, v = model._flip_forward(x, mg, plan.margin[r], self.shift_heatmap, plan.center[r], plan.scale[r])
            else:
                x, mg = model.input_buffers(cap, dev)
                ops.crop_clips(pool, plan.frame_idx[r], plan.M[r], out=x)
                mg.copy_(plan.margin[r])
                out = model._engine.run(x, mg, alias_outputs=True)          # consumed at once: no clones of the 7 outputs
                p, v = ops.get_final_preds(out[0], plan.center[r], plan.scale[r])
            preds.append(p)
            maxvals.append(v)
        if preds:
            p, v = torch.cat(preds)[:total], torch.cat(maxvals)[:total]
        else:
            nj = int(model.cfg.MODEL.NUM_JOINTS)
            p = torch.empty((0, nj, 2), dtype=torch.float32, device=dev)
            v = torch.empty((0, nj, 1), dtype=torch.float32, device=dev)
        return VideoPoseResult(p, v, plan.box_score[:total], plan.person_slot[:total], plan.pr_off, plan.center[:total],
                               plan.scale[:total])

    def detect_and_run(self, detector, pool, frame_number, num_frames, detect=None, max_persons=None):
        """``run`` on the boxes ``detector`` (a :class:`otpose_amd.PersonDetector`) finds in ``pool``."""
        boxes, scores, counts = detector.detect(pool)
        return self.run(pool, boxes, scores, counts, frame_number, num_frames, detect=detect, max_persons=max_persons)


def _slots_i32(x, device):
    """Per-slot integers as an int32 tensor on ``device`` (a host list is uploaded; a device tensor is taken as it is)."""
    if torch.is_tensor(x):
        return x
    return torch.as_tensor(x, dtype=torch.int32).to(device)
