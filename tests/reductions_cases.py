"""Inputs, torch-fp32 yardsticks and bounds shared by tests/test_reductions_host.py (CPU) and
tests/test_gpu_train_reductions.py (the kernels).  No GPU import.

The bound of a kernel output is 4 x the error of torch's own fp32 CPU kernels on the same operands against the float64
reference (a different but equally valid summation order, and an fp32 rstd), at least 4 ulp of the reference's largest
magnitude, and never more than the tolerance tests/test_gpu_train_ops.py already uses (3e-5 forward, 1e-4 gradients, both
relative to max(1, max|ref|))."""
import numpy as np
import torch

from tests import reductions_ref as R

FWD_TOL, GRAD_TOL = 3e-5, 1e-4
BF16 = torch.bfloat16


def gen(seed):
    return torch.Generator().manual_seed(seed)


def max_err(a, ref):
    a = a.detach().cpu().to(torch.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float((a - ref).abs().max()) if a.numel() else 0.0


def bound(yard, ref, cap_tol):
    refmax = float(ref.abs().max())
    floor = 4.0 * float(np.spacing(np.float32(refmax)))
    return min(max(4.0 * yard, floor), cap_tol * max(1.0, refmax))


# ---- BatchNorm fp32 --------------------------------------------------------------------------------------------------------
# (N, C, HW, expected slices S of the per-channel sums = otp_bn_workspace / (16 C))
# (2, 65, 4100): N * HW = 8200 >= 8192, so the split rule gives two slices; (2, 65, 4000) is the second 64-channel block of the
# finish kernels with one slice
BN_SMALL = [(1, 3, 1, 1), (4, 37, 108, 1), (2, 5, 4608, 2), (4, 3, 16640, 16), (2, 65, 4100, 2), (2, 65, 4000, 1)]
BN_LARGE = (1, 2048, 16700, 1)


def bn_inputs(n, c, hw, seed=0):
    """fp32 operands; the per-channel mean of x is up to three standard deviations either side (uniform: a normal offset
    reaches ten over 2048 channels, where E[x^2] - mean^2 loses two more digits than "a few" asks of it)."""
    g = gen(1000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)                                        # noqa: E731
    x = r(n, c, hw, 1) + 3.0 * (2 * torch.rand(1, c, 1, 1, generator=g) - 1)
    return {"x": x, "gamma": 1 + 0.1 * r(c), "beta": r(c), "res": r(n, c, hw, 1), "dy": r(n, c, hw, 1),
            "rm": 0.1 * r(c), "rv": r(c).abs() + 0.5}


def bn_forward_yardstick(d, relu, with_res, with_running, momentum=0.1, eps=1e-5):
    """torch's fp32 CPU batch norm on the same operands: y, mean, rstd, running statistics."""
    x = d["x"]
    rm, rv = (d["rm"].clone(), d["rv"].clone()) if with_running else (None, None)
    y, mean, rstd = torch.native_batch_norm(x, d["gamma"], d["beta"], rm, rv, True, momentum, eps)
    if with_res:
        y = y + d["res"]
    if relu:
        y = torch.relu(y)
    return {"y": y, "mean": mean, "rstd": rstd, "running_mean": rm, "running_var": rv}


def bn_backward_yardstick(d, y_mask, fwd, eps=1e-5):
    """torch's fp32 CPU batch-norm backward; ``y_mask``: the tensor whose sign is the ReLU mask (None: no ReLU)."""
    g = d["dy"] if y_mask is None else d["dy"] * (y_mask > 0).to(torch.float32)
    dx, dgamma, dbeta = torch.ops.aten.native_batch_norm_backward(g, d["x"], d["gamma"], None, None, fwd["mean"], fwd["rstd"],
                                                                  True, eps, [True, True, True])
    return {"dx": dx, "dres": g, "dgamma": dgamma, "dbeta": dbeta}


# ---- bf16 NHWC finalize / backward ----------------------------------------------------------------------------------------
FIN_ROWS = [1, 127, 128, 129, 385, 517, 2160]
FIN_CH = [(8, 8), (17, 24), (256, 256)]
# pixels -> rows of partial sums (otp_nhwc_bn_backward_workspace): one row, just under the 385 the unrolled loop needs, above it
NHWC_PIXELS = [(37, 1), (24570, 384), (33001, 516)]
NHWC_CH = [(8, 8), (17, 24)]


def finalize_inputs(rows, c, cs, seed=0):
    """fp32 partial sums (rows, 2, CS) as 64-pixel rows would give them: sum x and sum x*x with a positive variance."""
    g = gen(2000 + seed)
    k = 64.0
    mu, sig = 2.0 * torch.randn(cs, generator=g), 0.5 + torch.rand(cs, generator=g)
    a = mu + 0.3 * torch.randn(rows, cs, generator=g)
    q = a * a + sig * sig * (1 + 0.1 * torch.randn(rows, cs, generator=g))
    part = torch.stack([k * a, k * q], dim=1).to(torch.float32)
    return {"part": part, "count": rows * k, "gamma": 1 + 0.1 * torch.randn(c, generator=g),
            "beta": torch.randn(c, generator=g), "rm": 0.1 * torch.randn(c, generator=g),
            "rv": torch.rand(c, generator=g) + 0.5}


def finalize_yardstick(d, c, momentum=0.1, eps=1e-5):
    p, count = d["part"], torch.tensor(d["count"], dtype=torch.float32)
    cs = p.shape[2]
    mean = p[:, 0].sum(0) / count
    var = (p[:, 1].sum(0) / count - mean * mean).clamp_min(0)
    rstd = torch.rsqrt(var + eps)
    g, b = torch.zeros(cs), torch.zeros(cs)
    g[:c], b[:c] = d["gamma"], d["beta"]
    unb = var * count / (count - 1) if d["count"] > 1 else var
    return {"mean": mean, "rstd": rstd, "scale": g * rstd, "shift": b - mean * g * rstd,
            "running_mean": (1 - momentum) * d["rm"] + momentum * mean[:c],
            "running_var": (1 - momentum) * d["rv"] + momentum * unb[:c]}


def nhwc_bwd_inputs(pixels, c, cs, seed=0, eps=1e-5):
    """bf16 operands (pixels, CS), padding lanes zero.  |gy| is in [1, 1.5] with three signs in four positive, so that neither
    g - mean(g) - xhat * mean(g * xhat) nor its masked form -mean(g) - ... comes near zero: a gx element then sits well inside
    one bf16 interval unless it is within fp32 rounding of a boundary."""
    g = gen(3000 + seed)
    x = (torch.randn(pixels, cs, generator=g) + 2.0 * torch.randn(1, cs, generator=g)).to(BF16)
    sign = torch.where(torch.rand(pixels, cs, generator=g) < 0.75, 1.0, -1.0)
    gy = (sign * (1 + 0.5 * torch.rand(pixels, cs, generator=g))).to(BF16)
    y = torch.randn(pixels, cs, generator=g).to(BF16)
    x[:, c:], gy[:, c:], y[:, c:] = 0, 0, 0
    mean, _, rstd, _ = R.bn_stats(x.double().t().reshape(1, cs, pixels), eps)
    return {"x": x, "gy": gy, "y": y, "mean": mean.float(), "rstd": rstd.float(), "gamma": 1 + 0.1 * torch.randn(c, generator=g)}


def nhwc_bwd_yardstick(d, c, keep):
    g = d["gy"].float()
    if keep is not None:
        g = g * keep.float()
    x, count = d["x"].float(), float(g.shape[0])
    xh = (x - d["mean"]) * d["rstd"]
    s1, s2 = g.sum(0), (g * xh).sum(0)
    k1 = torch.zeros_like(s1)
    k1[:c] = d["gamma"] * d["rstd"][:c]
    return {"gx": (k1 * (g - s1 / count - xh * (s2 / count))).to(BF16), "gres": g.to(BF16), "dgamma": s2[:c], "dbeta": s1[:c]}


def bf16_ordinal(t):
    """bf16 values as integers that are consecutive for neighbouring values (sign-magnitude -> monotonic)."""
    b = t.detach().cpu().to(BF16).view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def bf16_mismatch(out, ref64):
    """(share of elements that differ from the bf16 rounding of ref64, largest difference in bf16 steps)."""
    diff = (bf16_ordinal(out) - bf16_ordinal(ref64.to(BF16))).abs()
    return float((diff > 0).double().mean()), int(diff.max())


BF16_ULP_SHARE = 1e-3


# ---- losses --------------------------------------------------------------------------------------------------------------------
LOSS_CASES = [(2, 17, 48, 8), (3, 17, 6912, 8), (1, 5, 300, 1), (4, 6, 257, 6), (300, 17, 64, 8), (2, 257, 48, 8),
              (1, 300, 100, 150)]
TOPK_GAP = 1e-3


def loss_inputs(b, j, hw, seed=0):
    """fp32 s, t, g (B, J, HW, 1), w (B, J, 1).  Joints with j % 3 != 0 carry one exact 1.0 somewhere in the batch (the others
    stay below 0.9): mixed flags.  About one weight in seven is zero.  The errors s - g and s - t of a (sample, joint) are noise
    scaled to an exact root mean square amp[b, j], a per-sample permutation of a geometric ladder, so that the per-sample losses
    a top-k ranks are well apart (asserted by the callers through reductions_ref.topk_gap).  Each sample's ladder has a factor of
    its own in [1, 2): with one ladder for all, every sample's top-k sum is the same number and the roundings of a sum over the
    samples all fall the same way, which measures that coincidence and not the kernel."""
    g_ = gen(4000 + seed)
    tgt = 0.9 * torch.rand(b, j, hw, generator=g_, dtype=torch.float64)
    for jj in range(j):
        if jj % 3:
            tgt[int(torch.randint(b, (1,), generator=g_)), jj, int(torch.randint(hw, (1,), generator=g_))] = 1.0
    ratio = 1.0 + 3.0 / j
    rank = torch.stack([torch.randperm(j, generator=g_) for _ in range(b)]).double()
    amp = (0.05 * ratio ** rank * (1 + torch.rand(b, 1, generator=g_, dtype=torch.float64))).reshape(b, j, 1)

    def noise():
        n = torch.randn(b, j, hw, generator=g_, dtype=torch.float64)
        return amp * n / n.pow(2).mean(2, keepdim=True).sqrt()

    s = tgt + noise()
    t = s - noise()
    w = (torch.rand(b, j, 1, generator=g_) > 0.15).float()
    w[:, 0] = 1.0
    return {"s": s.float().reshape(b, j, hw, 1), "t": t.float().reshape(b, j, hw, 1), "g": tgt.float().reshape(b, j, hw, 1),
            "w": w, "expected_flags": torch.tensor([1 if jj % 3 else 0 for jj in range(j)], dtype=torch.int32)}


def st_ohkw_yardstick(d, topk, flags):
    """The oracle's formulae through torch's fp32 CPU kernels and fp32 autograd."""
    from oracle import otpose_oracle as O
    s, t, g = (d[k].clone().requires_grad_() for k in ("s", "t", "g"))
    r = O.st_ohkw_mse_loss(s, t, g, d["w"], topk, global_flags=flags)
    gs, gt, gg = torch.autograd.grad(r["final_loss"], (s, t, g), allow_unused=True)
    out = {k: r[k].detach() for k in ("ohkm_loss_s", "mse_loss_s", "final_loss")}
    out.update(grad_s=gs, grad_t=torch.zeros_like(t) if gt is None else gt, grad_g=gg)
    return out


def joints_yardstick(d, topk, use_w, eff):
    from oracle import otpose_oracle as O
    j = d["s"].shape[1]
    w = d["w"] if use_w else torch.ones_like(d["w"])
    o = d["s"].clone().requires_grad_()
    r = O.joints_ohkm_mse_loss(o, d["g"], w, topk)
    (go,) = torch.autograd.grad(r["final_loss"], o)
    o2 = d["s"].clone().requires_grad_()
    v = O.joint_mse_loss(o2, d["g"], w) * j / (eff or j)
    (go2,) = torch.autograd.grad(v, o2)
    return {"ohkm_loss": r["ohkm_loss"].detach(), "mse_loss": r["mse_loss"].detach() * j / (eff or j),
            "final_loss": r["final_loss"].detach(), "grad_output": go, "plain": v.detach(), "plain_grad": go2}


# ---- gradient norm / AdamW -------------------------------------------------------------------------------------------------------
ADAMW_SIZES = [1, 3, 5, 1023, 1310723, 4200003]
SUMSQ_RTOL = 4 * 2.0 ** -24          # fp64 sums of four-element terms with three fp32 roundings each
P_TOL = 2e-6                         # the project's bound on the parameters, relative to max(1, max|p|)


def moment_rtol(beta):
    """exp_avg / exp_avg_sq relative to the tensor's max: the kernel forms 1 - beta from the float beta (a relative bias of
    at most 2^-24 beta / (1 - beta) against torch's double betas) plus eight fp32 roundings."""
    return 2.0 ** -24 * beta / (1.0 - beta) + 8 * 2.0 ** -24


def adamw_inputs(n, seed=0):
    g = gen(5000 + seed)
    return torch.randn(n, generator=g), [0.1 * torch.randn(n, generator=g) for _ in range(3)]
