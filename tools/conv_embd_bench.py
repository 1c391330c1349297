#!/usr/bin/env python
"""Time the conv embedding layer (csrc/convembd.hip) on the GPU: the fused forward launch and the backward in front of the
convolution's gradients, beside the same layer composed from launches that exist without it - ``otp_conv2d`` (exact-fp32 direct
kernel), ``otp_ln_channel`` and a ReLU pass (``torch.relu_``, an element-wise pass over the tensor).

    python tools/conv_embd_bench.py [--iters 200] [--warmup 20] [--out profiles/conv_embd_bench.txt]

Shapes: (16, 136, 96, 72) - one 136 -> 136 3x3 layer of a temporal encoder at the 384x288 configuration, 36.8 GFLOP - and
(16, 17, 96, 72), the flow encoder.  Every launch is timed by itself with device events, ``iters`` times after ``warmup``
launches of the same shape (weights packed once, outside the timed region); the table gives the median and the 10th / 90th
percentile in microseconds.  The rate column is 2 B T Cin Cout ks^2 FLOP over the median; 157.3 TFLOP/s is the fp32 matrix
peak of the MI355X.  HBM side of the fused forward: x read and y written = 2 B C T words, 120 MB, plus the 3.8 MB table (the
packed filter stays in L2)."""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from otpose_amd import hip, ops                      # noqa: E402

PEAK_F32_MFMA = 157.3e12
SHAPES = [(16, 136, 96, 72, 3), (16, 17, 96, 72, 3)]


def timed(fn, iters, warmup):
    """(median, p10, p90) in microseconds of ``fn``, each call between its own pair of device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2], t[len(t) // 10], t[(9 * len(t)) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_embd_bench needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda")
    L = hip.lib()
    fmt = "%-18s %-34s %9.1f %9.1f %9.1f %8s"
    lines = ["conv embedding layer, fp32, one launch per pair of device events, %d launches after %d (microseconds)" % (a.iters, a.warmup),
             "%-18s %-34s %9s %9s %9s %8s" % ("B,C,H,W,ks", "what", "median", "p10", "p90", "TFLOP/s")]
    for b, c, h, w, ks in SHAPES:
        t = h * w
        g = torch.Generator(device="cpu").manual_seed(c + ks)
        x = torch.randn(b, c, h, w, generator=g).to(dev)
        wt = (torch.randn(c, c, ks, ks, generator=g) * (c * ks * ks) ** -0.5).to(dev)
        gamma, beta = (1 + 0.1 * torch.randn(c, generator=g)).to(dev), (0.1 * torch.randn(c, generator=g)).to(dev)
        pe, go = torch.randn(c, t, generator=g).to(dev), torch.randn(b, c, t, generator=g).to(dev)
        out, z = torch.empty(b, c, t, device=dev), torch.empty(b, c, t, device=dev)
        st = hip.stream_of(x)
        packed = ops.pack_conv_embd_weight(wt)
        flop = 2.0 * b * t * c * c * ks * ks
        tag = f"{b},{c},{h},{w},{ks}"

        def row(what, tm, with_rate=False):
            lines.append(fmt % (tag, what, tm[0], tm[1], tm[2], "%.1f" % (flop / tm[0] / 1e6) if with_rate else "-"))
        args = ops.conv_embd_args(x, packed, None, gamma, beta, pe, out, None, c, ks, 1e-5)
        fused = timed(lambda: hip.check(L.otp_conv_embd(*args, st), "otp_conv_embd"), a.iters, a.warmup)
        row("fused forward", fused, True)
        args_z = ops.conv_embd_args(x, packed, None, gamma, beta, pe, out, z, c, ks, 1e-5)
        row("fused forward + z (training)", timed(lambda: hip.check(L.otp_conv_embd(*args_z, st), "otp_conv_embd"), a.iters, a.warmup),
            True)

        # the composed layer: otp_conv2d, otp_ln_channel, a ReLU pass (the table add rides on none of them: not counted)
        iv, zc = ops.View(x), torch.empty(b, c, h, w, device=dev)
        ov = ops.View(zc)
        d = ops.conv_desc(iv, ov, c, ks, ks, 1, ks // 2, 1, ops.ACT_NONE)
        wp = ops.pack_conv_weight(wt)
        conv = timed(lambda: ops.conv2d_launch(iv, wp, None, None, ov, d), a.iters, a.warmup)
        yc = torch.empty(b, c, t, device=dev)
        z3 = zc.view(b, c, t)
        ln = timed(lambda: hip.check(L.otp_ln_channel(hip.ptr(z3), hip.ptr(gamma), hip.ptr(beta), hip.ptr(yc), None, b, c, t, 1e-5,
                                                      st), "otp_ln_channel"), a.iters, a.warmup)
        relu = timed(lambda: torch.relu_(yc), a.iters, a.warmup)
        row("composed: otp_conv2d", conv, True)
        row("composed: otp_ln_channel", ln)
        row("composed: relu pass", relu)
        lines.append(fmt % (tag, "composed: sum of medians", conv[0] + ln[0] + relu[0], 0.0, 0.0, "-"))
        err = float((out - pe - yc).abs().max())           # faster and different is not faster
        assert err < 1e-4, err

        nbytes = L.otp_conv_embd_backward_pre_workspace(b, c, t)
        ws = torch.empty(nbytes // 4, device=dev)
        gz, gg, gb = torch.empty_like(z), torch.empty(c, device=dev), torch.empty(c, device=dev)
        row("backward_pre (grad_z, dgamma, dbeta)", timed(lambda: hip.check(L.otp_conv_embd_backward_pre(
            hip.ptr(z), None, hip.ptr(gamma), hip.ptr(beta), hip.ptr(go), hip.ptr(gz), hip.ptr(gg), hip.ptr(gb), hip.ptr(ws), nbytes,
            b, c, t, 1e-5, st), "otp_conv_embd_backward_pre"), a.iters, a.warmup))
        from otpose_amd import train_ops as T
        leaves = [x.clone().requires_grad_(), wt.clone().requires_grad_(), gamma.view(1, c, 1).clone().requires_grad_(),
                  beta.view(1, c, 1).clone().requires_grad_()]

        def step():
            for v in leaves:
                v.grad = None
            T.conv_embd(leaves[0], leaves[1], None, leaves[2], leaves[3], pe).backward(go)
        row("Function forward + backward", timed(step, max(10, a.iters // 10), 3))
        del leaves
        torch.cuda.empty_cache()
    lines.append("fp32 matrix peak %.1f TFLOP/s: 36.8 GFLOP -> %.0f us at (16,136,96,72,3); HBM side 2 B C T words = 120 MB" % (
        PEAK_F32_MFMA / 1e12, 2.0 * 16 * 6912 * 136 * 136 * 9 / PEAK_F32_MFMA * 1e6))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
