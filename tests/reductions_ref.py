"""Plain float64 references of the training step's reductions (no GPU import): BatchNorm2d in training mode with the fused
residual + ReLU and its backward, per-channel sums, the three heat-map losses with their gradients, the global gradient norm
with clip_grad_norm_'s coefficient, and AdamW.  Inputs of any float dtype are widened to float64 first, so a test hands in the
very fp32 / bf16 values a kernel read.  tests/test_reductions_host.py pins each of them against torch on the CPU."""
import math

import torch

from oracle import otpose_oracle as O


def _d(t):
    return None if t is None else t.detach().to(torch.float64)


# ---- BatchNorm2d, training mode -----------------------------------------------------------------------------------------
def bn_stats(x, eps=1e-5):
    """(mean, biased variance, rstd, count) per channel of x (N, C, ...)."""
    x = _d(x)
    n, c = x.shape[:2]
    xr = x.reshape(n, c, -1)
    count = n * xr.shape[2]
    mean = xr.mean(dim=(0, 2))
    var = ((xr - mean[None, :, None]) ** 2).mean(dim=(0, 2))
    return mean, var, 1.0 / torch.sqrt(var + eps), count


def bn_train_forward(x, gamma, beta, res=None, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, relu=True):
    """relu?(batch_norm(x) (+ res)) with batch statistics.  Returns a dict: y, mean, rstd, running_mean / running_var (the
    updated copies, None when not given; the variance that enters running_var is the unbiased one, and the biased one when
    there is a single value per channel)."""
    xd = _d(x)
    mean, var, rstd, count = bn_stats(xd, eps)
    shape = (1, -1) + (1,) * (xd.dim() - 2)
    y = (xd - mean.reshape(shape)) * rstd.reshape(shape) * _d(gamma).reshape(shape) + _d(beta).reshape(shape)
    if res is not None:
        y = y + _d(res)
    if relu:
        y = y.clamp_min(0.0)
    out = {"y": y, "mean": mean, "rstd": rstd, "running_mean": None, "running_var": None}
    if running_mean is not None:
        out["running_mean"] = (1.0 - momentum) * _d(running_mean) + momentum * mean
    if running_var is not None:
        unbiased = var * count / (count - 1.0) if count > 1 else var
        out["running_var"] = (1.0 - momentum) * _d(running_var) + momentum * unbiased
    return out


def bn_train_backward(dy, x, gamma, y=None, eps=1e-5):
    """Gradients of :func:`bn_train_forward`.  ``y`` is the forward's output when a ReLU followed (its mask is y > 0), else
    None.  Returns dx, dres (the gradient of the residual = the masked dy), dgamma, dbeta."""
    xd, g = _d(x), _d(dy)
    if y is not None:
        g = g * (y > 0).to(torch.float64)
    mean, _, rstd, count = bn_stats(xd, eps)
    shape = (1, -1) + (1,) * (xd.dim() - 2)
    red = (0,) + tuple(range(2, xd.dim()))
    xh = (xd - mean.reshape(shape)) * rstd.reshape(shape)
    dbeta = g.sum(dim=red)
    dgamma = (g * xh).sum(dim=red)
    dx = (_d(gamma) * rstd).reshape(shape) * (g - dbeta.reshape(shape) / count - xh * dgamma.reshape(shape) / count)
    return {"dx": dx, "dres": g, "dgamma": dgamma, "dbeta": dbeta}


def channel_sum(a):
    a = _d(a)
    return a.sum(dim=(0,) + tuple(range(2, a.dim())))


# ---- BatchNorm on the bf16 NHWC path: the two finalize steps ---------------------------------------------------------------
def nhwc_bn_finalize(part, c, count, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """part (rows, 2, CS): per-row sums of x and x*x.  Returns mean, rstd, scale, shift over all CS lanes (scale = shift = 0
    on the padding lanes c .. CS-1) and the updated running statistics over the c true channels."""
    p = _d(part)
    cs = p.shape[2]
    mean = p[:, 0].sum(0) / count
    var = (p[:, 1].sum(0) / count - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    g, b = torch.zeros(cs, dtype=torch.float64), torch.zeros(cs, dtype=torch.float64)
    g[:c], b[:c] = _d(gamma)[:c], _d(beta)[:c]
    out = {"mean": mean, "rstd": rstd, "scale": g * rstd, "shift": b - mean * g * rstd, "running_mean": None,
           "running_var": None}
    if running_mean is not None:
        unbiased = var * count / (count - 1.0) if count > 1 else var
        out["running_mean"] = (1.0 - momentum) * _d(running_mean) + momentum * mean[:c]
        out["running_var"] = (1.0 - momentum) * _d(running_var) + momentum * unbiased[:c]
    return out


def nhwc_bn_backward(gy, x, mean, rstd, gamma, c, keep=None):
    """gy, x (pixels, CS); mean, rstd (CS) as the kernel is handed them; ``keep`` (pixels, CS) bool: the ReLU mask, or None.
    Returns gx, gres (pixels, CS; gx = 0 on the padding lanes), dgamma, dbeta (c)."""
    g, xd = _d(gy), _d(x)
    if keep is not None:
        g = g * keep.to(torch.float64)
    count = g.shape[0]
    xh = (xd - _d(mean)) * _d(rstd)
    s1, s2 = g.sum(0), (g * xh).sum(0)
    k1 = torch.zeros_like(s1)
    k1[:c] = _d(gamma)[:c] * _d(rstd)[:c]
    return {"gx": k1 * (g - s1 / count - xh * (s2 / count)), "gres": g, "dgamma": s2[:c], "dbeta": s1[:c]}


# ---- heat-map losses (the oracle states the formulae; gradients by double autograd) ------------------------------------------
def st_ohkw_flags(g):
    """flags[j] = 1 when joint j has an exact 1.0 peak somewhere in the batch."""
    b, j = g.shape[:2]
    return (g.reshape(b, j, -1).amax(dim=(0, 2)) == 1).to(torch.int32)


def st_ohkw_per_sample(s, t, g, w, flags):
    """(B, J) per-sample per-joint losses that the top-k selection ranks."""
    b, j = s.shape[:2]
    s, t, g = (_d(v).reshape(b, j, -1) for v in (s, t, g))
    wv = _d(w).reshape(b, j, 1)
    a = s * wv
    dg, dt = (a - g * wv) ** 2, (a - t * wv) ** 2
    nf = (1 - flags.to(torch.float64)).reshape(1, j, 1)
    return (0.5 * (dg + nf * dt)).mean(2)


def st_ohkw(s, t, g, w, topk=8, flags=None):
    """ST_OHKW_MSELoss: the three scalars, the flags used, the gradients of final_loss w.r.t. s, t and g, and the per-sample
    losses."""
    b, j = s.shape[:2]
    sd, td, gd = (_d(v).requires_grad_() for v in (s, t, g))
    wd = _d(w).reshape(b, j, 1)
    fl = st_ohkw_flags(g) if flags is None else flags.to(torch.int32)
    r = O.st_ohkw_mse_loss(sd, td, gd, wd, topk, global_flags=fl)
    gs, gt, gg = torch.autograd.grad(r["final_loss"], (sd, td, gd), allow_unused=True)
    gt = torch.zeros_like(td) if gt is None else gt
    out = {k: r[k].detach() for k in ("ohkm_loss_s", "mse_loss_s", "final_loss")}
    out.update(flags=fl, grad_s=gs, grad_t=gt, grad_g=gg, per_sample=st_ohkw_per_sample(s, t, g, w, fl))
    return out


def joints_per_sample(o, g, w=None):
    b, j = o.shape[:2]
    o, g = _d(o).reshape(b, j, -1), _d(g).reshape(b, j, -1)
    wv = torch.ones(b, j, 1, dtype=torch.float64) if w is None else _d(w).reshape(b, j, 1)
    return (0.5 * (o * wv - g * wv) ** 2).mean(2)


def joints_ohkm_mse(o, g, w=None, effective_num_joints=None, topk=8):
    """JointsMSE_OHKMMSELoss: ohkm_loss, mse_loss (divided by effective_num_joints when given, else J), final_loss and its
    gradient w.r.t. o.  ``w`` None = no target weight."""
    b, j = o.shape[:2]
    od = _d(o).requires_grad_()
    wv = torch.ones(b, j, 1, dtype=torch.float64) if w is None else _d(w).reshape(b, j, 1)
    r = O.joints_ohkm_mse_loss(od, _d(g), wv, topk)
    (go,) = torch.autograd.grad(r["final_loss"], od)
    return {"ohkm_loss": r["ohkm_loss"].detach(), "mse_loss": r["mse_loss"].detach() * j / (effective_num_joints or j),
            "final_loss": r["final_loss"].detach(), "grad_output": go}


def joint_mse(o, g, w=None, effective_num_joints=None):
    """JointMSELoss: (value, gradient w.r.t. o)."""
    b, j = o.shape[:2]
    od = _d(o).requires_grad_()
    wv = torch.ones(b, j, 1, dtype=torch.float64) if w is None else _d(w).reshape(b, j, 1)
    v = O.joint_mse_loss(od, _d(g), wv) * j / (effective_num_joints or j)
    (go,) = torch.autograd.grad(v, od)
    return v.detach(), go


def topk_gap(per_sample, topk):
    """Smallest relative gap between the k-th and (k+1)-th largest loss of a sample (inf when topk == J)."""
    if topk >= per_sample.shape[1]:
        return math.inf
    v = torch.sort(per_sample, dim=1, descending=True).values
    return float(((v[:, topk - 1] - v[:, topk]) / v[:, topk - 1]).min())


# ---- gradient norm, clip coefficient, AdamW ------------------------------------------------------------------------------------
def grad_sumsq(grads):
    return sum(float((_d(g) ** 2).sum()) for g in grads)


def clip_coef(norm, max_norm):
    """clip_grad_norm_: gradients are multiplied by min(1, max_norm / (norm + 1e-6)); no clipping when max_norm <= 0."""
    return min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0


def adamw_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, clip=1.0):
    """One torch.optim.AdamW step (decoupled decay, bias corrections from the double betas) on float64 copies;
    ``step`` is the 1-based count of this step.  Returns the new (p, exp_avg, exp_avg_sq)."""
    b1, b2 = betas
    p, g, m, v = _d(p), _d(g) * clip, _d(m), _d(v)
    p = p * (1.0 - lr * weight_decay)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v
