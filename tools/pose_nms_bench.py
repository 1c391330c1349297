#!/usr/bin/env python
"""Times of the pose NMS (``ops.pose_nms``, ``PoseTrackEvaluator(nms=...)``) on the seeded synthetic case of 3 000 frames and
on one ten times larger, both with a detector's duplicates added (``synthetic.pose_nms_case``): kernel time of otp_pose_nms,
hard and soft, and of otp_pose_assign in the same run as the yardstick (HIP events around 20 launches each after a warm-up),
wall time of ``assign()`` with and without the NMS, and wall time of the numpy restatement (tests/pose_nms_ref.py) on the
same packed arrays on the host.  Each case runs in a child process of its own under a time limit.  Prints one JSON line per
case.  No threshold: the figures go into DESIGN.md section 3.10.

    python tools/pose_nms_bench.py [--frames 3000 30000] [--launches 20] [--timeout 240]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from otpose_amd import hip, ops, posetrack_eval as PE, synthetic as S      # noqa: E402
from tests import pose_nms_ref as R                                        # noqa: E402

IN_VIS, OKS_THRE = 0.2, 0.9                                                # Base_PoseTrack17.yaml


def events_ms(fn, launches):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def wall_ms(fn, repeats):
    best = math.inf
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def run(frames, launches):
    gt_frames, preds, box, fid, area, _ = S.pose_nms_case(frames, 7)
    g = PE.pack_ground_truth(gt_frames)
    pr_off, pr_sample = PE.pack_predictions(g["frame_map"], fid, len(g["kept"]))
    host = [pr_off, pr_sample, np.ascontiguousarray(preds[:, :, :2]), np.ascontiguousarray(preds[:, :, 2:]), box, area]
    dev = [torch.from_numpy(a).cuda() for a in host]
    npr, f, n = int(pr_sample.size), int(pr_off.size - 1), int(preds.shape[0])
    keep, score, rank = ops.pose_nms(*dev, oks_thresh=OKS_THRE, in_vis_thre=IN_VIS)        # warm-up: library load
    keep8 = torch.empty(npr, dtype=torch.int8, device="cuda")
    sig = (ctypes.c_double * 17)(*ops.COCO_SIGMAS)
    L, P = hip.lib(), hip.ptr

    # the kernel alone: the C entry point, without the wrapper's host-side checks
    def nms(mode):
        return lambda: L.otp_pose_nms(*[P(a) for a in dev], sig, IN_VIS, OKS_THRE, math.nan, mode, 20, P(keep8), P(score),
                                      P(rank), None, f, npr, n, hip.stream_of(keep8))

    hard_ms, gauss_ms, linear_ms = (events_ms(nms(m), launches) for m in (0, 1, 2))
    gt = [torch.from_numpy(g[k]).cuda() for k in PE._GT_KEYS]
    labels, scores, ngt = ops.pose_assign(*dev[:5], *gt)
    assign_ms = events_ms(lambda: L.otp_pose_assign(*[P(a) for a in (*dev[:5], *gt)], 0.5, P(labels), P(scores), P(ngt), f, npr,
                                                    n, gt[1].shape[0], hip.stream_of(labels)), launches)

    xy, mv = dev[2], dev[3]
    plain = PE.PoseTrackEvaluator(g)
    plain.add(xy, mv, box, fid)
    with_nms = PE.PoseTrackEvaluator(g, nms=PE.PoseNMS(oks_thresh=OKS_THRE, in_vis_thre=IN_VIS))
    with_nms.add(xy, mv, box, fid, area=area)
    plain.assign(), with_nms.assign()                                                      # warm-up: ground truth upload
    plain_wall, nms_wall = wall_ms(plain.assign, 5), wall_ms(with_nms.assign, 5)

    numpy_hard = numpy_soft = math.inf
    for _ in range(3):
        t = time.perf_counter()
        want = R.pose_nms_ref(*host, oks_thresh=OKS_THRE, in_vis_thre=IN_VIS)
        numpy_hard = min(numpy_hard, time.perf_counter() - t)
        t = time.perf_counter()
        R.pose_nms_ref(*host, oks_thresh=OKS_THRE, in_vis_thre=IN_VIS, soft=True)
        numpy_soft = min(numpy_soft, time.perf_counter() - t)
    nms(0)()
    torch.cuda.synchronize()
    return {
        "frames": frames, "kept_frames": f, "predicted_persons": npr, "persons_kept_hard": int(want[0].sum()),
        "device": torch.cuda.get_device_name(0), "pose_nms_hard_kernel_ms": round(hard_ms, 4),
        "pose_nms_soft_gaussian_kernel_ms": round(gauss_ms, 4), "pose_nms_soft_linear_kernel_ms": round(linear_ms, 4),
        "pose_assign_kernel_ms": round(assign_ms, 4), "assign_wall_ms": round(plain_wall, 3),
        "assign_with_nms_wall_ms": round(nms_wall, 3), "numpy_hard_wall_ms": round(numpy_hard * 1e3, 3),
        "numpy_soft_wall_ms": round(numpy_soft * 1e3, 3),
        "keep_equals_numpy": bool(np.array_equal(keep8.cpu().numpy().astype(bool), want[0])),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[3000, 30000])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--case", type=int, help="run this one case in this process")
    a = ap.parse_args()
    if a.case is not None:
        if not torch.cuda.is_available():
            raise SystemExit("pose_nms_bench needs the GPU")
        print(json.dumps(run(a.case, a.launches)), flush=True)
        return
    for f in a.frames:                                                   # a case that fails or runs out of time ends the run
        subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(f), "--launches", str(a.launches)],
                       check=True, timeout=a.timeout)


if __name__ == "__main__":
    main()
