#!/usr/bin/env python
"""Time the local-window attention (csrc/localattn.hip) on the GPU: forward and backward in microseconds with the bytes each
must move and the rate that gives, beside an eager PyTorch evaluation of the same banded formula and ``otp_chan_attn`` at the
same shape.

    python tools/local_attn_bench.py [--iters 50] [--warmup 10] [--out profiles/local_attn_bench.txt]

Shapes: (16, 136, T', 2 heads) for T' in {6912, 3456, 1728} (the three pyramid levels at the 384x288 configuration) with windows
9 and 19, and (16, 17, 6912, 1 head) (the flow encoder).  Times are device events around ``iters`` back-to-back launches after
``warmup`` launches of the same shape, best of three such windows; bytes are counted from the shapes:

    forward   q, k, v read + out written                                            4 B C T words
    backward  q, k, v, dO, P read + dq, dk, dv written (the necessary traffic)       (7 C + W nh) B T words
              the two-pass form reads dO twice and P twice and writes and reads dS: (8 C + 4 W nh) B T words are what it moves

The rate column divides the NECESSARY bytes by the time; 6.29 TB/s is the copy rate of the MI355X."""
from __future__ import annotations

import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from otpose_amd import hip, ops                      # noqa: E402

COPY_RATE = 6.29e12
SHAPES = [(16, 136, t, 2, w) for t in (6912, 3456, 1728) for w in (9, 19)] + [(16, 17, 6912, 1, 9), (16, 17, 6912, 1, 19)]


def timed(fn, iters, warmup):
    """Best-of-three mean time in microseconds of ``fn`` over ``iters`` back-to-back calls (device events)."""
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
        best = min(best, a.elapsed_time(b) * 1e3 / iters)
    return best


def eager_band(q, k, v, n_head, window, scale, rel):
    """The banded formula with PyTorch-ROCm operators: shifted products, one per band position."""
    b, c, t = q.shape
    hs, w = c // n_head, window // 2
    qh, kh, vh = (x.view(b, n_head, hs, t) for x in (q, k, v))
    kp = torch.nn.functional.pad(kh, (w, w))
    vp = torch.nn.functional.pad(vh, (w, w))
    s = torch.stack([(qh * kp[..., j:j + t]).sum(2) for j in range(window)], -1) * scale          # (B, nh, T, W)
    if rel is not None:
        s = s + rel.view(1, n_head, 1, window)
    pos = torch.arange(t, device=q.device)[:, None] + torch.arange(window, device=q.device)[None, :] - w
    p = torch.softmax(s.masked_fill((pos < 0) | (pos >= t), float("-inf")), -1)
    out = torch.zeros_like(qh)
    for j in range(window):
        out = out + p[..., j].unsqueeze(2) * vp[..., j:j + t]
    return out.reshape(b, c, t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("local_attn_bench needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda")
    L = hip.lib()
    lines = ["local-window attention, fp32, device-event times, best of 3 windows of %d launches (microseconds)" % a.iters,
             "%-26s %9s %8s %6s | %9s %8s %6s | %10s %10s | %9s" % ("B,C,T,nh,window", "fwd us", "fwd MB", "TB/s", "bwd us", "bwd MB",
                                                                   "TB/s", "eager fwd", "eager bwd", "chan_attn")]
    for b, c, t, nh, win in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(t + win)
        q, k, v, go = (torch.randn(b, c, t, generator=g).to(dev) for _ in range(4))
        rel = (0.1 * torch.randn(1, 1, nh, win, generator=g)).to(dev)
        scale = 1.0 / math.sqrt(c // nh)
        reltab = rel.reshape(nh, win).contiguous()
        out = torch.empty_like(q)
        probs = torch.empty(b * nh, t, win, device=dev)
        st = hip.stream_of(q)
        args = ops.local_attn_args(q, k, v, reltab, out, None, nh, win, scale)
        fwd = timed(lambda: hip.check(L.otp_local_attn(*args, st), "otp_local_attn"), a.iters, a.warmup)
        hip.check(L.otp_local_attn(*ops.local_attn_args(q, k, v, reltab, out, probs, nh, win, scale), st), "otp_local_attn")
        nbytes = L.otp_local_attn_backward_workspace(b, c, t, nh, win)
        ws = torch.empty(nbytes // 4, device=dev)
        gq, gk, gv, grel = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q), torch.empty_like(reltab)
        bwd = timed(lambda: hip.check(L.otp_local_attn_backward(
            hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(probs), hip.ptr(go), hip.ptr(gq), hip.ptr(gk), hip.ptr(gv), hip.ptr(grel),
            hip.ptr(ws), nbytes, b, c, t, nh, win, scale, st), "otp_local_attn_backward"), a.iters, a.warmup)
        fwd_b = 4 * b * c * t * 4
        bwd_b = (7 * c + win * nh) * b * t * 4
        e_it = max(3, a.iters // 10)
        efwd = timed(lambda: eager_band(q, k, v, nh, win, scale, rel), e_it, 2)
        leaves = [x.clone().requires_grad_() for x in (q, k, v)]

        def eager_step():
            for x in leaves:
                x.grad = None
            eager_band(*leaves, nh, win, scale, rel).backward(go)
        eboth = timed(eager_step, e_it, 2)
        chan = timed(lambda: ops.chan_attn(q, k, v, nh, scale), a.iters, a.warmup)
        # the native results against the eager formula at the timed size (faster and different is not faster)
        err = float((out - eager_band(q, k, v, nh, win, scale, rel)).abs().max())
        assert err < 1e-4, err
        lines.append("%-26s %9.1f %8.1f %6.2f | %9.1f %8.1f %6.2f | %10.1f %10.1f | %9.1f" % (
            f"{b},{c},{t},{nh},{win}", fwd, fwd_b / 1e6, fwd_b / fwd / 1e6, bwd, bwd_b / 1e6, bwd_b / bwd / 1e6, efwd,
            eboth - efwd, chan))
        del leaves
        torch.cuda.empty_cache()
    lines.append("floors at %.2f TB/s: fwd 240.6 MB -> %.1f us at (16,136,6912); eager bwd = (fwd + bwd) - fwd" % (
        COPY_RATE / 1e12, 240.6e6 / COPY_RATE * 1e6))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
