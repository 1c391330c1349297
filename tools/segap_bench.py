#!/usr/bin/env python
"""Time of ``ANETdetection.evaluate`` at a validation-epoch size - 200 videos x 200 kept predictions x 20 classes, T = 5 tIoU
thresholds - with predictions that are already device tensors (the output of ``batched_nms_videos``), against the same metric
on the host, and of the two kernels of csrc/segap.hip on their own.

The host side is tests/segap_ref.py's ``detection_ap`` (numpy: one tIoU row and one ranking per prediction), not the
reference's ``metrics.py``, which loops over a pandas data frame with ``iterrows`` and needs pandas and joblib: the figure is
what an interpreter costs on this work, and the reference's loop costs more per prediction, not less.  Every timed call ends in
a device synchronisation (``evaluate`` returns host numbers, the kernel loops are followed by one).  Prints one JSON line.

    python tools/segap_bench.py [--videos 200] [--preds 200] [--classes 20] [--iters 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from otpose_amd import ops, segmetrics                         # noqa: E402
from tests import segap_ref as R                               # noqa: E402


def make_case(n_videos, n_preds, n_classes, seed=0):
    """Ground truth: 4 .. 12 segments per video in 1 .. 3 of the classes; predictions: jittered copies of them with a label
    of the video's classes (most) or any class, float32 values."""
    rs = np.random.RandomState(seed)
    gt = {"video-id": [], "t-start": [], "t-end": [], "label": []}
    preds = {"video-id": [], "t-start": [], "t-end": [], "label": [], "score": []}
    for v in range(n_videos):
        vid = f"v{v:04d}"
        m = rs.randint(4, 13)
        classes = rs.choice(n_classes, rs.randint(1, 4), replace=False)
        start = np.cumsum(rs.uniform(5, 60, m))
        seg = np.stack([start, start + rs.uniform(3, 40, m)], 1)
        label = classes[rs.randint(0, len(classes), m)]
        gt["video-id"] += [vid] * m
        gt["t-start"] += seg[:, 0].tolist()
        gt["t-end"] += seg[:, 1].tolist()
        gt["label"] += label.tolist()
        pick = rs.randint(0, m, n_preds)
        p = seg[pick] + rs.uniform(-0.6, 0.6, (n_preds, 2)) * (seg[pick, 1] - seg[pick, 0])[:, None]
        plabel = np.where(rs.uniform(0, 1, n_preds) < 0.7, label[pick], rs.randint(0, n_classes, n_preds))
        preds["video-id"] += [vid] * n_preds
        preds["t-start"] += p[:, 0].tolist()
        preds["t-end"] += p[:, 1].tolist()
        preds["label"] += plabel.tolist()
    n = len(preds["label"])
    preds["score"] = (np.linspace(0.001, 0.99, n) + rs.uniform(-0.3, 0.3, n) * 0.989 / n)[rs.permutation(n)]
    for table in (gt, preds):
        for k in table:
            if k != "video-id":
                table[k] = np.asarray(table[k], np.int64 if k == "label" else np.float32)
    return gt, preds


def median_ms(fn, iters):
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=200)
    ap.add_argument("--preds", type=int, default=200)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "segap_bench needs the GPU"
    thr = np.linspace(0.1, 0.5, 5)
    gt, host = make_case(a.videos, a.preds, a.classes)
    gpu = {k: (v if k == "video-id" else torch.from_numpy(v).cuda()) for k, v in host.items()}
    det = segmetrics.ANETdetection(None, tiou_thresholds=thr, ground_truth=gt, dataset_name="bench")

    def run_gpu():
        return det.evaluate(gpu, verbose=False)

    def run_host():
        table = {k: (v if k == "video-id" else v.cpu().numpy()) for k, v in gpu.items()}
        return R.detection_ap(gt, table, thr)

    # the kernels alone, on the tables evaluate() builds for this input
    t = {k: torch.from_numpy(v).cuda() for k, v in R.kernel_tables(gt, host, thr).items() if k != "ap"}
    reps = 50

    def run_match():
        for _ in range(reps):
            m = ops.seg_ap_match(t["pred_seg"], t["pred_offsets"], t["gt_seg"], t["gt_offsets"], thr)
        return m

    def run_ap():
        for _ in range(reps):
            x = ops.seg_ap(t["match"], t["order"], t["class_offsets"], t["npos"])
        return x

    for _ in range(3):
        run_gpu()
        run_match()
        run_ap()
    want = run_host()[0]
    run_gpu()
    same_match = bool(torch.equal(run_match(), t["match"]))
    result = {"videos": a.videos, "preds_per_video": a.preds, "classes": a.classes, "thresholds": len(thr),
              "groups": int(t["pred_offsets"].shape[0] - 1), "ground_truths": int(t["gt_seg"].shape[0]),
              "evaluate_ms": round(median_ms(run_gpu, a.iters), 3),
              "host_numpy_ms": round(median_ms(run_host, a.host_iters), 1),
              "seg_ap_match_us": round(median_ms(run_match, a.iters) * 1e3 / reps, 2),
              "seg_ap_us": round(median_ms(run_ap, a.iters) * 1e3 / reps, 2),
              "max_abs_ap_deviation_from_host": float(np.abs(det.ap - want).max()), "same_match_as_host": same_match,
              "average_mAP": float(det.ap.mean(axis=1).mean())}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
