#!/usr/bin/env python
"""Time the token x token attention (csrc/tokattn.hip) on the GPU: forward and forward + backward in milliseconds, the
algorithmic TFLOP/s that gives and its share of the fp32-matrix peak, beside ``torch.nn.functional.scaled_dot_product_attention``
on the same operands.

    python tools/token_attn_bench.py [--iters 10] [--warmup 3] [--dropout P] [--products half] [--out profiles/token_attn_bench.txt]

``--products half`` adds, per shape, a row for the half-operand kernels (csrc/tokattn_h.hip): their times, the ratio of the fp32
kernels' time to theirs, the ratio of SDPA's time to theirs, and their largest difference from SDPA's output.

``--dropout P`` (0 < P < 1) adds, per shape, the times of the ``_dropout`` entry points at rate P beside the p = 0 times of the
same run: what the in-kernel mask (8 hashes per lane and key tile forward and in backward pass A, 16 in pass B) costs.

Shapes: (16, 136, 6912) with 2 heads (head width 68) and with 8 heads (head width 17).  Times are device events around ``iters``
back-to-back calls after ``warmup`` calls of the same shape, best of three such windows.  FLOP are counted from the shapes:
forward 4 B T^2 C (S and P V), forward + backward 14 B T^2 C (the algorithmic count: S, dP, dq, dk, dv on top of the forward; the
two-pass backward forms S and dP in both passes, work the count does not credit).  157.3 TFLOP/s is the fp32-matrix peak of the
MI355X.  The SDPA
baseline gets its operands in its own (B, heads, T, hd) layout, made outside the timed region."""
from __future__ import annotations

import argparse
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from otpose_amd import hip                           # noqa: E402

PEAK = 157.3e12
SHAPES = [(16, 136, 2, 6912), (16, 136, 8, 6912)]


def timed(fn, iters, warmup):
    """Best-of-three mean time in milliseconds of ``fn`` over ``iters`` back-to-back calls (device events)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / iters)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.0, help="also time the dropout entry points at this rate")
    ap.add_argument("--products", choices=("f32", "half"), default="f32",
                    help="half: add a row per shape with the half-operand kernels beside the fp32 and SDPA columns")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not 0.0 <= a.dropout < 1.0:
        raise SystemExit("--dropout takes a rate in [0, 1)")
    if not torch.cuda.is_available():
        raise SystemExit("token_attn_bench needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda")
    L = hip.lib()
    lines = ["token x token attention, fp32, device-event times, best of 3 windows of %d calls (milliseconds)" % a.iters,
             "%-18s %8s %7s %6s | %9s %7s %6s | %9s %11s | %9s" % ("B,C,nh,T", "fwd ms", "TFLOP/s", "peak", "f+b ms", "TFLOP/s",
                                                                   "peak", "sdpa fwd", "sdpa f+b", "max|diff|")]
    for b, c, nh, t in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(t + nh)
        q, k, v, go = (torch.randn(b, c, t, generator=g).to(dev) for _ in range(4))
        scale = 1.0 / math.sqrt(c // nh)
        out, lse = torch.empty_like(q), torch.empty(b, nh, t, device=dev)
        gq, gk, gv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        ws = torch.empty(L.otp_token_attn_workspace(b, nh, t, c // nh) // 4, device=dev)
        st = hip.stream_of(q)
        P = hip.ptr

        def fwd(keep_lse=False):
            hip.check(L.otp_token_attn_forward(P(q), P(k), P(v), None, P(out), P(lse) if keep_lse else None, b, c, nh, t, scale, st),
                      "otp_token_attn_forward")

        def both():
            fwd(True)
            hip.check(L.otp_token_attn_backward(P(q), P(k), P(v), None, P(out), P(lse), P(go), P(gq), P(gk), P(gv), P(ws), b, c, nh,
                                                t, scale, st), "otp_token_attn_backward")
        t_fwd, t_both = timed(fwd, a.iters, a.warmup), timed(both, a.iters, a.warmup)

        seed = 0x123456789ABCDEF

        def fwd_drop(keep_lse=False):
            hip.check(L.otp_token_attn_forward_dropout(P(q), P(k), P(v), None, P(out), P(lse) if keep_lse else None, b, c, nh, t,
                                                       scale, a.dropout, seed, st), "otp_token_attn_forward_dropout")

        def both_drop():
            fwd_drop(True)
            hip.check(L.otp_token_attn_backward_dropout(P(q), P(k), P(v), None, P(out), P(lse), P(go), P(gq), P(gk), P(gv), P(ws),
                                                        b, c, nh, t, scale, a.dropout, seed, st), "otp_token_attn_backward_dropout")
        if a.dropout > 0.0:
            d_fwd, d_both = timed(fwd_drop, a.iters, a.warmup), timed(both_drop, a.iters, a.warmup)

        # --products half: the half-operand kernels (csrc/tokattn_h.hip) on the same operands, the same timing method
        def fwd_half(keep_lse=False):
            hip.check(L.otp_token_attn_forward_h1(P(q), P(k), P(v), None, P(out), P(lse) if keep_lse else None, b, c, nh, t, scale,
                                                  0.0, 0, None, st), "otp_token_attn_forward_h1")

        ws_h = torch.empty(L.otp_token_attn_h1_workspace(b, nh, t, c // nh) // 4, device=dev)

        def both_half():
            fwd_half(True)
            hip.check(L.otp_token_attn_backward_h1(P(q), P(k), P(v), None, P(out), P(lse), P(go), P(gq), P(gk), P(gv), P(ws_h), b, c,
                                                   nh, t, scale, 0.0, 0, None, st), "otp_token_attn_backward_h1")
        if a.products == "half":
            h_fwd, h_both = timed(fwd_half, a.iters, a.warmup), timed(both_half, a.iters, a.warmup)
            fwd_half()
            h_out = out.clone()

        # the baseline in its own layout (B, heads, T, hd)
        sq, sk, sv, sgo = (x.view(b, nh, c // nh, t).transpose(2, 3).contiguous() for x in (q, k, v, go))
        e_it = max(2, a.iters // 3)
        s_fwd = timed(lambda: F.scaled_dot_product_attention(sq, sk, sv, scale=scale), e_it, 1)
        leaves = [x.clone().requires_grad_() for x in (sq, sk, sv)]

        def sdpa_step():
            for x in leaves:
                x.grad = None
            F.scaled_dot_product_attention(*leaves, scale=scale).backward(sgo)
        s_both = timed(sdpa_step, e_it, 1)
        with torch.no_grad():
            ref = F.scaled_dot_product_attention(sq, sk, sv, scale=scale).transpose(2, 3).reshape(b, c, t)
        fwd()
        diff = float((out - ref).abs().max())
        assert diff < 1e-4, diff                                     # faster and different is not faster
        f_fwd, f_both = 4.0 * b * t * t * c, 14.0 * b * t * t * c
        lines.append("%-18s %8.2f %7.1f %5.1f%% | %9.2f %7.1f %5.1f%% | %9.2f %11.2f | %9.1e" % (
            f"{b},{c},{nh},{t}", t_fwd, f_fwd / t_fwd / 1e9, 100 * f_fwd / t_fwd / 1e-3 / PEAK, t_both, f_both / t_both / 1e9,
            100 * f_both / t_both / 1e-3 / PEAK, s_fwd, s_both, diff))
        if a.dropout > 0.0:
            lines.append("%-18s %8.2f %7s %5.2fx | %9.2f %7s %5.2fx | dropout p = %g against the p = 0 row above" % (
                "", d_fwd, "", d_fwd / t_fwd, d_both, "", d_both / t_both, a.dropout))
        if a.products == "half":
            h_diff = float((h_out - ref).abs().max())
            assert h_diff < 1e-2, h_diff
            lines.append("%-18s %8.2f %7.1f %5.2fx | %9.2f %7.1f %5.2fx | %9.2f %11.2f | %9.1e  half products: x = f32 time / half "
                         "time, then sdpa time / half time" % ("  products=half", h_fwd, f_fwd / h_fwd / 1e9, t_fwd / h_fwd, h_both,
                                                               f_both / h_both / 1e9, t_both / h_both, s_fwd / h_fwd,
                                                               s_both / h_both, h_diff))
        del leaves, sq, sk, sv, sgo, ref
        torch.cuda.empty_cache()
    lines.append("FLOP: forward 4 B T^2 C, forward + backward 14 B T^2 C; peak %.1f TFLOP/s (fp32 matrix)" % (PEAK / 1e12))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
