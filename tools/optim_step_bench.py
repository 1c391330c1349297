#!/usr/bin/env python
"""Time one launch of otp_sgd_step and of otp_adamw_step on the same flat buffers, at the three group sizes that
``make_optimizer(OTPose(cfg2()))`` yields (HRNet-W48: decay / no-decay / pretrained), clip on.

Device events around blocks of launches, the two kernels alternating block by block; printed per size: the median and the
spread of the microseconds per launch and the bytes/s the algorithm's traffic implies (SGD with momentum reads p, g, buf and
writes p, buf = 20 B per element; AdamW reads p, g, m, v and writes p, m, v = 28 B per element).

    python tools/optim_step_bench.py [--blocks 7] [--launches 50]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from otpose_amd import OTPose, cfg2, hip, make_optimizer        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time on a CPU"
    opt = make_optimizer(OTPose(cfg2()), cfg2(), fused=False)
    sizes = [sum(p.numel() for p in g["params"]) for g in opt.param_groups]
    del opt
    L = hip.lib()
    acc = torch.zeros(1 + int(L.otp_grad_sumsq_scratch()), dtype=torch.float64, device="cuda")
    for name, n in zip(("decay", "no_decay", "pretrained"), sizes):
        gen = torch.Generator(device="cuda").manual_seed(1)
        p = torch.randn(n, device="cuda", generator=gen)
        g = torch.randn(n, device="cuda", generator=gen) * 1e-3
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        st = hip.stream_of(p)
        acc[:1].zero_()
        hip.check(L.otp_grad_sumsq(hip.ptr(g), n, hip.ptr(acc), st), "otp_grad_sumsq")
        step = [0]

        def sgd():
            hip.check(L.otp_sgd_step(hip.ptr(p), hip.ptr(g), hip.ptr(m), n, 1e-6, 0.9, 0.0, 0.01, 0, 0, hip.ptr(acc), 1.0, st),
                      "otp_sgd_step")

        def adamw():
            step[0] += 1
            hip.check(L.otp_adamw_step(hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v), n, 1e-6, 0.9, 0.999, 1e-8, 0.01, step[0],
                                       hip.ptr(acc), 1.0, st), "otp_adamw_step")

        times = {"sgd": [], "adamw": []}
        for fn in (sgd, adamw) * 3:                       # warm-up
            fn()
        torch.cuda.synchronize()
        for _ in range(args.blocks):
            for key, fn in (("sgd", sgd), ("adamw", adamw)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[key].append(1e3 * e0.elapsed_time(e1) / args.launches)
        assert bool(torch.isfinite(p).all())
        for key, per in (("sgd", 20), ("adamw", 28)):
            med = statistics.median(times[key])
            print("%-10s n %9d  %-5s %8.1f us/launch (min %.1f max %.1f over %d blocks of %d)  %5.0f GB/s at %d B/element"
                  % (name, n, key, med, min(times[key]), max(times[key]), args.blocks, args.launches, per * n / med / 1e3, per))
        del p, g, m, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
