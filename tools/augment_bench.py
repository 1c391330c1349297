#!/usr/bin/env python
"""Timing of the training blur fused into the crop (csrc/crop.hip) at cfg2 batch 16: ``ops.crop_clips`` cutting 16
persons x 5 frames of 384 x 288 from a seeded 20-frame 720p pool with the blur off (the plain kernel), on half of the
80 slots and on all of them (HIP events on the launch stream over ``--iters`` launches after a warm-up).  For scale, the
host cost of the reference's way - torchvision 0.8's blur restated on torch ``conv2d`` - per 720p frame on the CPU
threads torch uses (``--cpu-frames`` frames, 0 = skip)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from otpose_amd import augment as A  # noqa: E402
from otpose_amd import crop as C  # noqa: E402
from otpose_amd import ops  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from crop_bench import ev  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--cpu-frames", type=int, default=3)
    a = ap.parse_args()
    assert a.iters >= 50
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs the GPU")
    B, F, W, H, S = a.batch, 5, 288, 384, 20
    rng = np.random.RandomState(0)
    pool_np = rng.randint(0, 256, (S, 720, 1280, 3)).astype(np.uint8)
    pool = torch.from_numpy(pool_np).cuda()
    boxes = np.stack([rng.uniform(0, 1100, B), rng.uniform(0, 500, B), rng.uniform(60, 300, B),
                      rng.uniform(100, 500, B)], axis=1)
    c, s = C.box_to_center_scale(boxes, W / H, 1.25)
    M = torch.from_numpy(C.crop_matrix(c, s, rng.uniform(-30, 30, B), (W, H))).cuda()
    fi = torch.from_numpy(rng.randint(0, S, (B, F)).astype(np.int32)).cuda()
    flip = torch.from_numpy(rng.randint(0, 2, B).astype(np.uint8)).cuda()
    out = torch.empty((B, 3 * F, H, W), dtype=torch.float32, device="cuda")
    blur = torch.from_numpy(np.stack([[A.blur_table(v) for v in row] for row in rng.uniform(0.1, 5, (B, F))])).cuda()
    half = torch.from_numpy((np.arange(B * F).reshape(B, F) % 2).astype(np.uint8)).cuda()
    every = torch.ones((B, F), dtype=torch.uint8, device="cuda")

    res = {"shape": [B, 3 * F, H, W], "pool": list(pool.shape), "iters": a.iters}
    res["plain_us"] = round(ev(lambda: ops.crop_clips(pool, fi, M, flip, out=out), a.iters), 2)
    res["blur_off_us"] = round(ev(lambda: ops.crop_clips(pool, fi, M, flip, out=out, blur=blur,
                                                         blur_on=torch.zeros_like(every)), a.iters), 2)
    res["blur_half_us"] = round(ev(lambda: ops.crop_clips(pool, fi, M, flip, out=out, blur=blur, blur_on=half),
                                   a.iters), 2)
    res["blur_all_us"] = round(ev(lambda: ops.crop_clips(pool, fi, M, flip, out=out, blur=blur, blur_on=every),
                                  a.iters), 2)
    for k in ("plain", "blur_off", "blur_half", "blur_all"):
        print("%-10s %8.1f us" % (k, res[k + "_us"]))
    if a.cpu_frames > 0:
        t = torch.from_numpy(A.blur_table(2.5)).expand(720, 1, 9, 5).contiguous()
        times = []
        for k in range(a.cpu_frames + 1):
            x = torch.from_numpy(pool_np[k % S]).unsqueeze(0).float()
            t0 = time.perf_counter()
            y = torch.nn.functional.conv2d(torch.nn.functional.pad(x, [2, 2, 4, 4], mode="reflect"), t, groups=720)
            torch.round(y).to(torch.uint8)
            times.append(time.perf_counter() - t0)
        res["cpu_conv2d_ms_per_720p_frame"] = round(1e3 * float(np.median(times[1:])), 2)
        res["cpu_threads"] = torch.get_num_threads()
        print("host torchvision-0.8 blur: %.1f ms per 720p frame (%d threads)"
              % (res["cpu_conv2d_ms_per_720p_frame"], res["cpu_threads"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
