#!/usr/bin/env python
"""Time of ``batched_nms_videos`` at the ActionFormer post-processing size - 16 videos x 2000 segments x 20 classes, soft
(gaussian) multiclass NMS, iou 0.1, min_score 0.001, max_seg_num 200 - against the same work done the way the reference does
it: device tensors to the host, a Python loop over the classes of each video, an O(n^2) loop per class, results back.

The host side is tests/segnms_ref.py's ``batched_nms`` (numpy, the arithmetic of a round over arrays, ``np.exp`` in place
of the per-element C ``expf``), not the reference's compiled extension, which is not part of this repository: its rounds are
numpy calls, so it is slower than compiled C by what an interpreter costs.  Prints one JSON line.

    python tools/segnms_bench.py [--videos 16] [--segs 2000] [--classes 20] [--iters 20]
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

from otpose_amd import segnms                                  # noqa: E402
from tests import segnms_ref as R                              # noqa: E402


def make_videos(n_videos, n_segs, n_classes, seed=0):
    rs = np.random.RandomState(seed)
    videos = []
    for _ in range(n_videos):
        c, l = rs.uniform(0, 2304, n_segs), rs.uniform(4, 200, n_segs)
        segs = np.stack([c - l / 2, c + l / 2], 1).astype(np.float32)
        videos.append((segs, rs.uniform(0.001, 0.99, n_segs).astype(np.float32), rs.randint(0, n_classes, n_segs).astype(np.int64)))
    return videos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=16)
    ap.add_argument("--segs", type=int, default=2000)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=2)
    a = ap.parse_args()
    kw = dict(use_soft_nms=True, multiclass=True, sigma=0.5, voting_thresh=0.7)
    host = make_videos(a.videos, a.segs, a.classes)
    gpu = [tuple(torch.from_numpy(x).cuda() for x in v) for v in host]

    def run_gpu():
        return segnms.batched_nms_videos(gpu, 0.1, 0.001, 200, **kw)

    def run_loop():                                            # one call per video, still one launch for its classes
        return [segnms.batched_nms(*v, 0.1, 0.001, 200, **kw) for v in gpu]

    def run_host():
        out = []
        for v in gpu:
            s, p, c = (t.cpu().numpy() for t in v)
            out.append(tuple(torch.from_numpy(x).cuda() for x in R.batched_nms(s, p, c, 0.1, 0.001, 200, **kw)))
        return out

    def median_ms(fn, iters):
        times = []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times))

    for _ in range(3):
        run_gpu()
        run_loop()
    R._expf = np.exp                                           # the vectorised form (see the module docstring)
    ref, got = run_host(), run_gpu()
    same_classes = all(torch.equal(r[2], g[2]) for r, g in zip(ref, got))
    result = {"videos": a.videos, "segs": a.segs, "classes": a.classes,
              "batched_nms_videos_ms": round(median_ms(run_gpu, a.iters), 3),
              "batched_nms_per_video_ms": round(median_ms(run_loop, a.iters), 3),
              "host_numpy_per_class_loop_ms": round(median_ms(run_host, a.host_iters), 1),
              "kept_per_video": int(got[0][1].shape[0]), "same_classes_as_host": bool(same_classes)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
