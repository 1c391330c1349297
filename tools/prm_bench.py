#!/usr/bin/env python
"""Time the RSN attention kernels (csrc/prm.hip) on the GPU: ``otp_prm_gate`` + ``otp_prm_apply`` - everything of RSN_ATTENTION
behind its leading 3x3 layer - beside the same part of the eager PyTorch-ROCm module (``nn.Conv2d`` / ``nn.BatchNorm2d`` in eval
mode, as model/RSB.py:192-203 composes them), and one training forward + backward of the whole module through ``TrainGraph``.

    python tools/prm_bench.py [--iters 200] [--warmup 20] [--out profiles/prm_bench.txt]

Shapes: (16, 17, 96, 72) and (16, 32, 96, 72), the two chains of the 384x288 configuration.  Every entry is timed by itself with
device events, ``iters`` times after ``warmup`` runs; the table gives the median and the 10th / 90th percentile in microseconds.
The HBM column is what the launch has to move - f read and out written, 2 N C H W words, for the apply launch; f read once for
the gate - over the median, against the 8 TB/s of the MI355X: a launch far below that rate at these sizes is bound by latency
(launch, a dependent chain inside the workgroup), not by HBM."""
from __future__ import annotations

import argparse
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from otpose_amd import hip, ops                      # noqa: E402
from otpose_amd import modules as M                  # noqa: E402
from otpose_amd import train as TR                   # noqa: E402
from otpose_amd import train_ops as T                # noqa: E402

SHAPES = [(16, 17, 96, 72), (16, 32, 96, 72)]
HBM = 8.0e12


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


def fill(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in mod.state_dict().items():
            if k.endswith("num_batches_tracked"):
                continue
            if k.endswith("running_var"):
                v.copy_(0.8 + 0.4 * torch.rand(v.shape, generator=g))
            elif v.dim() == 4:
                v.copy_(torch.randn(v.shape, generator=g) * (2.0 / (v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5)
            elif k.endswith("bn.weight"):
                v.copy_(1 + 0.1 * torch.randn(v.shape, generator=g))
            else:
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
    return mod


class EagerTail(nn.Module):
    """RSN_ATTENTION behind its 3x3 layer as PyTorch runs it (RSB.py:195-202), sharing the container's parameters."""

    def __init__(self, m):
        super().__init__()
        self.m = m

    @staticmethod
    def cbr(layer, x):
        return torch.relu(layer.bn(layer.conv(x)))

    def forward(self, f):
        m = self.m
        a = torch.sigmoid(self.cbr(m.conv_bn_relu_prm_2_2, self.cbr(m.conv_bn_relu_prm_2_1, f.mean((2, 3), keepdim=True))))
        s = torch.sigmoid(self.cbr(m.conv_bn_relu_prm_3_2, self.cbr(m.conv_bn_relu_prm_3_1, f)))
        return f * (1 + a * s)


class Holder(nn.Module):
    def __init__(self, blk):
        super().__init__()
        self.b, self.cfg = blk, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prm_bench needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda")
    L = hip.lib()
    fmt = "%-14s %-40s %9.1f %9.1f %9.1f %8s"
    lines = ["RSN attention behind its 3x3 layer, fp32, one entry per pair of device events, %d runs after %d (microseconds)"
             % (a.iters, a.warmup), "%-14s %-40s %9s %9s %9s %8s" % ("N,C,H,W", "what", "median", "p10", "p90", "TB/s")]
    for n, c, h, w in SHAPES:
        mod = fill(M.RSN_ATTENTION(c), c).to(dev).eval()
        f = torch.relu(torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(c + 1))).to(dev)
        st = hip.stream_of(f)
        l21, l22 = ops.prm_layer(mod.conv_bn_relu_prm_2_1, c, dev), ops.prm_layer(mod.conv_bn_relu_prm_2_2, c, dev)
        l31, l32 = ops.prm_layer(mod.conv_bn_relu_prm_3_1, c, dev), ops.prm_layer(mod.conv_bn_relu_prm_3_2, 81, dev)
        gate, out = torch.empty(n, c, 1, 1, device=dev), torch.empty_like(f)
        gargs, aargs = ops.prm_gate_args(f, l21, l22, gate, False), ops.prm_apply_args(f, gate, l31, l32, out)
        tag, words = f"{n},{c},{h},{w}", n * c * h * w

        def row(what, tm, nbytes=None):
            lines.append(fmt % (tag, what, tm[0], tm[1], tm[2], "%.2f" % (nbytes / tm[0] / 1e6) if nbytes else "-"))
        tg = timed(lambda: hip.check(L.otp_prm_gate(*gargs, st), "otp_prm_gate"), a.iters, a.warmup)
        ta = timed(lambda: hip.check(L.otp_prm_apply(*aargs, st), "otp_prm_apply"), a.iters, a.warmup)

        def both():
            hip.check(L.otp_prm_gate(*gargs, st), "otp_prm_gate")
            hip.check(L.otp_prm_apply(*aargs, st), "otp_prm_apply")
        row("otp_prm_gate (mean + two 1x1 + sigmoid)", tg, 4.0 * words)
        row("otp_prm_apply (1x1, 9x9, gates, product)", ta, 8.0 * words)
        row("gate + apply, back to back", timed(both, a.iters, a.warmup), 12.0 * words)
        eager = EagerTail(mod)
        with torch.no_grad():
            ref = eager(f)
            err = float((out - ref).abs().max())
            assert err < 1e-4 * max(1.0, float(ref.abs().max())), err              # faster and different is not faster
            row("eager PyTorch module (same part)", timed(lambda: eager(f), a.iters, a.warmup))

        # one training forward + backward of the whole module (3x3 layer included), batch statistics
        holder = Holder(fill(M.RSN_ATTENTION(c), c)).to(dev).train()
        holder.train_dropout = False
        x = torch.randn(n, c, h, w, device=dev)
        go = torch.randn(n, c, h, w, device=dev)

        def step():
            holder.zero_grad(set_to_none=True)
            graph = TR.TrainGraph(holder)
            xg = x.clone().requires_grad_()
            with T.active_routes(graph.routes):
                graph.rsn_attention("b", xg).backward(go)
        row("TrainGraph.rsn_attention fwd + bwd", timed(step, max(10, a.iters // 10), 3))
        ref_mod = fill(M.RSN_ATTENTION(c), c).to(dev).train()
        full = EagerTail(ref_mod)

        def eager_step():
            ref_mod.zero_grad(set_to_none=True)
            xg = x.clone().requires_grad_()
            full(EagerTail.cbr(ref_mod.conv_bn_relu_prm_1, xg)).backward(go)
        row("eager PyTorch module fwd + bwd", timed(eager_step, max(10, a.iters // 10), 3))
        del holder, ref_mod
        torch.cuda.empty_cache()
    lines.append("HBM 8.0 TB/s: f read + out written = %.1f MB at C = 17 (%.1f us), %.1f MB at C = 32 (%.1f us)" % (
        8 * 16 * 17 * 6912 / 1e6, 8 * 16 * 17 * 6912 / HBM * 1e6, 8 * 16 * 32 * 6912 / 1e6, 8 * 16 * 32 * 6912 / HBM * 1e6))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(text + "\n")


if __name__ == "__main__":
    main()
