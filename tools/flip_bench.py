#!/usr/bin/env python
"""Timing of the flip test at cfg2 batch 16: the three kernels (``ops.crop_clips(mirror_pair=True)``, ``ops.mirror_pair``,
``ops.flip_test_merge``) next to the plain crop, then ``OTPose.predict`` without and with ``flip_test`` and the peak memory
of the B and the 2B engine.  HIP events on the launch stream over ``--iters`` launches after a warm-up (``--predict-iters``
for the two predict loops); prints microseconds per call and, for the kernels, the bytes each call must move."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from otpose_amd import OTPose, cfg2, ops  # noqa: E402
from otpose_amd import crop as C  # noqa: E402
from otpose_amd import synthetic as S  # noqa: E402


def ev(fn, iters, warm=5):
    for _ in range(warm):
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
    ap.add_argument("--predict-iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    a = ap.parse_args()
    assert a.iters >= 50
    if not torch.cuda.is_available():
        raise SystemExit("flip_bench needs the GPU")
    cfg = cfg2()
    B, F, S_ = a.batch, 5, 20
    W, H = cfg.MODEL.IMAGE_SIZE
    w, h = cfg.MODEL.HEATMAP_SIZE
    J = cfg.MODEL.NUM_JOINTS
    rng = np.random.RandomState(0)
    pool = torch.from_numpy(rng.randint(0, 256, (S_, 720, 1280, 3)).astype(np.uint8)).cuda()
    boxes = np.stack([rng.uniform(0, 1100, B), rng.uniform(0, 500, B), rng.uniform(60, 300, B),
                      rng.uniform(100, 500, B)], axis=1)
    c, s = C.box_to_center_scale(boxes, W / H, 1.25)
    M = torch.from_numpy(C.crop_matrix(c, s, 0.0, (W, H))).cuda()
    fi = torch.from_numpy(rng.randint(0, S_, (B, F)).astype(np.int32)).cuda()
    plain = torch.empty((B, 3 * F, H, W), dtype=torch.float32, device="cuda")
    pair = torch.empty((2 * B, 3 * F, H, W), dtype=torch.float32, device="cuda")
    hm = torch.randn((2 * B, J, h, w), generator=torch.Generator().manual_seed(1)).cuda()
    cc, ss = torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda()
    ops.crop_clips(pool, fi, M, out=plain)

    res = {"batch": B, "clip": [3 * F, H, W], "heatmaps": [2 * B, J, h, w], "iters": a.iters}
    t = {
        "crop_us": ev(lambda: ops.crop_clips(pool, fi, M, out=plain), a.iters),
        "pair_crop_us": ev(lambda: ops.crop_clips(pool, fi, M, out=pair, mirror_pair=True), a.iters),
        "mirror_pair_us": ev(lambda: ops.mirror_pair(plain, out=pair), a.iters),
        "flip_decode_us": ev(lambda: ops.flip_test_merge(hm, shift_heatmap=True, center=cc, scale=ss), a.iters),
    }
    bytes_ = {"crop_us": (plain.numel() * 4, pool.numel()), "pair_crop_us": (pair.numel() * 4, pool.numel()),
              "mirror_pair_us": (pair.numel() * 4, plain.numel() * 4),
              "flip_decode_us": (B * J * h * w * 4, hm.numel() * 4)}
    for k, v in t.items():
        wr, rd = bytes_[k]
        res[k] = round(v, 2)
        res[k.replace("_us", "_bytes")] = wr + rd
        print("%-16s %9.1f us  %.2f TB/s (%.1f MB written + %s%.1f MB read)"
              % (k[:-3], v, (wr + rd) / (v * 1e-6) / 1e12, wr / 1e6, "at most " if "crop" in k else "", rd / 1e6))

    if not a.no_model:
        model = OTPose(cfg)
        S.fill_synthetic_(model)
        model = model.cuda().eval()
        margin = torch.tensor([[1.0, 1.0, 2.0, 2.0]] * B)
        with torch.no_grad():
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t_plain = ev(lambda: model.predict(pool, fi, c, s, margin), a.predict_iters, warm=3)
            peak_b = torch.cuda.max_memory_allocated() - base
            model.invalidate_engine()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t_flip = ev(lambda: model.predict(pool, fi, c, s, margin, flip_test=True, shift_heatmap=True),
                        a.predict_iters, warm=3)
            peak_2b = torch.cuda.max_memory_allocated() - base
            # one switch back to the plain predict: the B engine is rebuilt (its first call, graph capture included)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model.predict(pool, fi, c, s, margin)
            e1.record()
            e1.synchronize()
            t_switch = e0.elapsed_time(e1) * 1e3
        res.update({"predict_us": round(t_plain, 1), "predict_flip_us": round(t_flip, 1),
                    "predict_flip_ratio": round(t_flip / t_plain, 3), "switch_rebuild_us": round(t_switch, 1),
                    "peak_bytes_B_engine": peak_b, "peak_bytes_2B_engine": peak_2b, "predict_iters": a.predict_iters})
        print("predict          %9.1f us" % t_plain)
        print("predict flip     %9.1f us  (x%.2f)" % (t_flip, t_flip / t_plain))
        print("switch + rebuild %9.1f us" % t_switch)
        print("peak memory      B engine %.2f GB, 2B engine %.2f GB" % (peak_b / 2 ** 30, peak_2b / 2 ** 30))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
