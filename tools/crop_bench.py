#!/usr/bin/env python
"""Timing of the crop kernel (csrc/crop.hip) at cfg2 batch 16: ``ops.crop_clips`` cutting 16 persons x 5 frames of
384 x 288 from a seeded 20-frame 720p pool, next to ``ops.frames_to_clip`` on the same number of pre-cut uint8 crops.
HIP events on the launch stream over ``--iters`` launches after a warm-up; prints microseconds per call and the
bytes per second of the bytes each call must move (fp32 written + uint8 read, the pool counted once)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from otpose_amd import crop as C  # noqa: E402
from otpose_amd import ops  # noqa: E402


def ev(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters):
        fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    assert a.iters >= 50
    if not torch.cuda.is_available():
        raise SystemExit("crop_bench needs the GPU")
    B, F, W, H, S = a.batch, 5, 288, 384, 20
    rng = np.random.RandomState(0)
    pool = torch.from_numpy(rng.randint(0, 256, (S, 720, 1280, 3)).astype(np.uint8)).cuda()
    boxes = np.stack([rng.uniform(0, 1100, B), rng.uniform(0, 500, B), rng.uniform(60, 300, B),
                      rng.uniform(100, 500, B)], axis=1)
    c, s = C.box_to_center_scale(boxes, W / H, 1.25)
    M = torch.from_numpy(C.crop_matrix(c, s, rng.uniform(-30, 30, B), (W, H))).cuda()
    fi = torch.from_numpy(rng.randint(0, S, (B, F)).astype(np.int32)).cuda()
    out = torch.empty((B, 3 * F, H, W), dtype=torch.float32, device="cuda")
    crops = torch.from_numpy(rng.randint(0, 256, (B, F, H, W, 3)).astype(np.uint8)).cuda()

    t_crop = ev(lambda: ops.crop_clips(pool, fi, M, out=out), a.iters)
    t_norm = ev(lambda: ops.frames_to_clip(crops, out=out), a.iters)
    written = out.numel() * 4
    res = {
        "shape": [B, 3 * F, H, W], "pool": list(pool.shape), "iters": a.iters,
        "crop_clips_us": round(t_crop, 2),
        "crop_clips_bytes_per_s": (written + pool.numel()) / (t_crop * 1e-6),
        "frames_to_clip_us": round(t_norm, 2),
        "frames_to_clip_bytes_per_s": (written + crops.numel()) / (t_norm * 1e-6),
        "bytes_written": written, "pool_bytes": pool.numel(), "crop_bytes": crops.numel(),
    }
    print("crop_clips      %8.1f us  %.2f TB/s (%.1f MB written + at most %.1f MB read)"
          % (t_crop, res["crop_clips_bytes_per_s"] / 1e12, written / 1e6, pool.numel() / 1e6))
    print("frames_to_clip  %8.1f us  %.2f TB/s (%.1f MB written + %.1f MB read)"
          % (t_norm, res["frames_to_clip_bytes_per_s"] / 1e12, written / 1e6, crops.numel() / 1e6))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
