#!/usr/bin/env python
"""Times of the PoseTrack AP evaluation (otpose_amd.posetrack_eval) on the seeded synthetic case of 3 000 frames and on one
ten times larger: kernel time of otp_pose_assign and otp_ap_curve (HIP events around 20 launches each after a warm-up),
wall time of ``PoseTrackEvaluator.summarize()`` (host packing + upload + both kernels + the torch sort + the read-back),
and wall time of the vectorised numpy restatement (tests/posetrack_ap_ref.py) on the same packed arrays on the host.
Prints one JSON line per case.  No threshold: the figures go into DESIGN.md section 3.9.

    python tools/posetrack_ap_bench.py [--frames 3000 30000] [--launches 20]
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

from otpose_amd import ops, posetrack_eval as PE, synthetic as S     # noqa: E402
from tests import posetrack_ap_ref as R                               # noqa: E402


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


def run(frames, launches):
    gt_frames, preds, box, fid = S.posetrack_eval_case(frames, 7, crowded=(5, frames // 2), big_polygon=(9, frames // 2))
    t = time.perf_counter()
    g = PE.pack_ground_truth(gt_frames)
    t_pack_gt = time.perf_counter() - t
    ev = PE.PoseTrackEvaluator(g)
    p = torch.from_numpy(preds).cuda()
    ev.add(p[:, :, :2].contiguous(), p[:, :, 2:].contiguous(), box, fid)
    ev.summarize()                                                   # warm-up: library load, ground truth upload
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = ev.summarize()
        walls.append(time.perf_counter() - t)

    pr_off, pr_sample = PE.pack_predictions(g["frame_map"], fid, len(g["kept"]))
    host = [pr_off, pr_sample, preds[:, :, :2], preds[:, :, 2:], box] + [g[k] for k in PE._GT_KEYS]
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in host]
    # the kernels alone: the C entry points, without the wrappers' host-side checks
    from otpose_amd import hip
    labels, scores, ngt = ops.pose_assign(*dev)
    L, P = hip.lib(), hip.ptr
    n_pr, n, n_gt = dev[1].numel(), dev[2].shape[0], dev[6].shape[0]
    mv = dev[3].contiguous()
    assign_ms = events_ms(lambda: L.otp_pose_assign(*[P(a) for a in (dev[0], dev[1], dev[2], mv, *dev[4:])], 0.5, P(labels),
                                                    P(scores), P(ngt), len(g["kept"]), n_pr, n, n_gt,
                                                    hip.stream_of(labels)), launches)
    lab, off, _ = ops.sort_entries(labels, scores)
    total = ngt.sum(0, dtype=torch.int64)
    out = torch.zeros((15, 3), dtype=torch.float64, device="cuda")
    curve_ms = events_ms(lambda: L.otp_ap_curve(P(lab), P(off), P(total), P(out), None, None, 15, hip.stream_of(lab)),
                         launches)
    sort_ms = events_ms(lambda: ops.sort_entries(labels, scores), 5)

    numpy_walls = []
    for _ in range(3):
        t = time.perf_counter()
        l, s, m = R.pose_assign_ref(*host)
        t_assign = time.perf_counter() - t
        want = R.ap_curve_ref(l, s, m)
        numpy_walls.append((time.perf_counter() - t, t_assign))
    diff = max(float(np.abs(res[k] - w).max()) for k, w in zip(("ap", "precision", "recall"), want))
    return {
        "frames": frames, "kept_frames": int(len(g["kept"])), "predicted_persons": int(n_pr), "gt_persons": int(n_gt),
        "entries_per_joint_max": int((off[1:] - off[:-1]).max()), "device": torch.cuda.get_device_name(0),
        "pose_assign_kernel_ms": round(assign_ms, 4), "ap_curve_kernel_ms": round(curve_ms, 4),
        "sort_entries_ms": round(sort_ms, 4), "summarize_wall_ms": round(min(walls) * 1e3, 3),
        "numpy_restatement_wall_ms": round(min(w for w, _ in numpy_walls) * 1e3, 3),
        "numpy_assign_wall_ms": round(min(a for _, a in numpy_walls) * 1e3, 3),
        "pack_ground_truth_once_ms": round(t_pack_gt * 1e3, 3), "mean_ap": res["table"]["Mean"],
        "max_abs_diff_vs_numpy": diff,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[3000, 30000])
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("posetrack_ap_bench needs the GPU")
    for f in a.frames:
        print(json.dumps(run(f, a.launches)), flush=True)


if __name__ == "__main__":
    main()
