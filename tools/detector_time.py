#!/usr/bin/env python
"""Per-stage time of the person detector at 416 x 416 on the GPU: launch count and, per frame, the letterbox, the
convolutions, the activation passes, the head decode and the NMS at 300 candidates, for batch 1 and 16.

    python tools/detector_time.py [--batches 1 16] [--iters 20] [--frame 1080 1920]

Device events around each stage's launches, replayed ``--iters`` times after a warm-up; seeded weights (the times do not
depend on the values).  Prints one JSON line per batch size.  Needs the GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from otpose_amd import detector as DET     # noqa: E402
from otpose_amd import hip, ops            # noqa: E402


def timed(fn, iters):
    """Milliseconds per call of ``fn`` (device events; 3 warm-up calls)."""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def nms_case(batch, n_rows, n_cand, classes, rs):
    """(batch, n_rows, 5 + classes) predictions with ``n_cand`` rows above the threshold in 30 clusters of 10."""
    pred = np.zeros((batch, n_rows, 5 + classes), np.float32)
    pred[..., 4] = rs.uniform(0.0, 0.3, (batch, n_rows))
    pred[..., :4] = rs.uniform(20, 380, (batch, n_rows, 4))
    pred[..., 5:] = rs.uniform(0, 1, (batch, n_rows, classes))
    for b in range(batch):
        rows = rs.permutation(n_rows)[:n_cand]
        centers = rs.uniform(40, 376, (30, 2))
        for k, r in enumerate(rows):
            pred[b, r, :2] = centers[k % 30] + rs.uniform(-3, 3, 2)
            pred[b, r, 2:4] = (60, 120) + rs.uniform(-3, 3, 2)
            pred[b, r, 4] = rs.uniform(0.45, 0.99)
            pred[b, r, 5] = 0.99
    return torch.from_numpy(pred)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frame", type=int, nargs=2, default=[1080, 1920])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detector_time.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    model = DET.PersonDetector().to(dev)
    for p in model.parameters():
        p.data.normal_(0, 0.01)
    lib = hip.lib()
    for batch in args.batches:
        frames = torch.from_numpy(rs.randint(0, 256, (batch, *args.frame, 3)).astype(np.uint8)).to(dev)
        x = ops.letterbox(frames, 416)
        model(x)
        eng = model._engine
        stream = hip.stream_of(x)
        kinds = {"conv": (lib.otp_conv2d, "otp_conv2d"), "pass": (lib.otp_leaky_pass, "otp_leaky_pass"),
                 "decode": (lib.otp_yolo_decode, "otp_yolo_decode")}

        def stage(kind):
            fn, name = kinds[kind]
            steps = [s for s in eng.steps if s[0] == kind]

            def run():
                for s in steps:
                    hip.check(fn(*s[1], stream), name)
            return run, len(steps)

        res = {"batch": batch, "frame": args.frame, "img_size": 416}
        res["letterbox_ms"] = timed(lambda: ops.letterbox(frames, 416, out=x), args.iters) / batch
        for kind, key in (("conv", "convs"), ("pass", "passes"), ("decode", "decode")):
            run, n = stage(kind)
            res[key + "_launches"] = n
            res[key + "_ms"] = timed(run, args.iters) / batch
        pred = nms_case(batch, model.num_rows, 300, model.num_classes, rs).to(dev)
        ws = torch.empty(lib.otp_box_nms_merge_workspace(batch, model.num_rows) // 4, dtype=torch.int32, device=dev)
        res["nms300_ms"] = timed(lambda: ops.box_nms_merge(pred, 0.4, 0.4, tuple(args.frame), 416, 0, ws), args.iters) / batch
        res["launches"] = 1 + eng.launches + 1
        res["forward_ms"] = timed(lambda: model(x), args.iters) / batch
        res["detect_ms"] = timed(lambda: model.detect(frames), args.iters) / batch
        res["passes_over_convs"] = res["passes_ms"] / res["convs_ms"]
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
        del frames, x, pred, ws
        model.invalidate_engine()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
