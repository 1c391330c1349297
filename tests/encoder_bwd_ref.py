"""Plain float64 restatements of the temporal encoders' small operators with their gradients written out by hand (no GPU
import, no autograd inside), and beside each the fp32 yardstick: the same operation under torch's fp32 CPU autograd on the same
operands (the pattern of tests/reductions_ref.py / tests/reductions_cases.py).  Inputs of any float dtype are widened to float64
first, so a test hands in the very fp32 values a kernel read.  Written from the reference model's definitions: channel LayerNorm
(model/blocks.py:95-110), the depthwise q / k / v convs (:359-381), channel attention (:427-447), MaxPool1d(3, 2, 1) (:234-238),
nn.Upsample(linear) and the nearest up-sampling of the HRNet fuse rows.  tests/test_encoder_bwd_host.py pins every restatement
against torch's float64 autograd of the same expression."""
import math

import torch
import torch.nn.functional as F


def _d(t):
    return None if t is None else t.detach().to(torch.float64)


def _autograd(fn, inputs, grad_out):
    """(output, gradients) of ``fn`` under torch autograd in the dtype of ``inputs``."""
    leaves = [t.detach().clone().requires_grad_() for t in inputs]
    out = fn(*leaves)
    grads = torch.autograd.grad(out, leaves, grad_out.to(out.dtype))
    return out.detach(), [g.detach() for g in grads]


# ---- channel LayerNorm of (B, C, T) ---------------------------------------------------------------------------------------
def layer_norm_expr(x, gamma, beta, eps=1e-5):
    mu = x.mean(1, keepdim=True)
    r = x - mu
    return r / torch.sqrt((r ** 2).mean(1, keepdim=True) + eps) * gamma.reshape(1, -1, 1) + beta.reshape(1, -1, 1)


def layer_norm(x, gamma, beta, dy, eps=1e-5):
    """y, dx, dgamma (C), dbeta (C) and dyxh = dy * xhat (what otp_ln_channel_backward writes for a later channel sum)."""
    x, g, b, dy = _d(x), _d(gamma).reshape(1, -1, 1), _d(beta).reshape(1, -1, 1), _d(dy)
    mu = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    xh = (x - mu) * rstd
    dyg = dy * g
    dx = rstd * (dyg - dyg.mean(1, keepdim=True) - xh * (dyg * xh).mean(1, keepdim=True))
    return {"y": xh * g + b, "dx": dx, "dgamma": (dy * xh).sum(dim=(0, 2)), "dbeta": dy.sum(dim=(0, 2)), "dyxh": dy * xh}


def layer_norm_yardstick(x, gamma, beta, dy, eps=1e-5):
    y, (dx, dg, db) = _autograd(lambda a, g, b: layer_norm_expr(a, g, b, eps), [x, gamma, beta], dy)
    # dy * xhat with torch's fp32 mean / sqrt, as the forward expression forms xhat
    mu = x.mean(1, keepdim=True)
    r = x - mu
    xh = r / torch.sqrt((r ** 2).mean(1, keepdim=True) + eps)
    return {"y": y, "dx": dx, "dgamma": dg.reshape(-1), "dbeta": db.reshape(-1), "dyxh": dy * xh}


# ---- depthwise Conv1d(C, C, 3, stride, padding 1, groups C, no bias) ------------------------------------------------------
def dwconv3_out_len(t, stride):
    return (t + 2 - 3) // stride + 1


def dwconv3(x, w, dy, stride, prefill=None):
    """y, dx, dw (C, 1, 3); ``prefill``: what the weight gradient's destination held before (the kernel accumulates)."""
    x, w, dy = _d(x), _d(w).reshape(-1, 3), _d(dy)
    b, c, t = x.shape
    to = dwconv3_out_len(t, stride)
    xp = F.pad(x, (1, 1))
    taps = [xp[:, :, k: k + stride * (to - 1) + 1: stride] for k in range(3)]       # x[to * s - 1 + k]
    y = sum(w[:, k].reshape(1, c, 1) * taps[k] for k in range(3))
    dw = torch.stack([(dy * taps[k]).sum(dim=(0, 2)) for k in range(3)], dim=1)
    dxp = torch.zeros_like(xp)
    for k in range(3):
        dxp[:, :, k: k + stride * (to - 1) + 1: stride] += w[:, k].reshape(1, c, 1) * dy
    dw = dw.reshape(c, 1, 3)
    if prefill is not None:
        dw = dw + _d(prefill)
    return {"y": y, "dx": dxp[:, :, 1: t + 1], "dw": dw}


def dwconv3_yardstick(x, w, dy, stride, prefill=None):
    c = x.shape[1]
    y, (dx, dw) = _autograd(lambda a, k: F.conv1d(a, k, None, stride, 1, 1, c), [x, w], dy)
    return {"y": y, "dx": dx, "dw": dw if prefill is None else prefill + dw}


# ---- channel attention -----------------------------------------------------------------------------------------------------
def chan_attn_expr(q, k, v, n_head, scale):
    b, c, _ = q.shape
    hs = c // n_head
    qq, kk, vv = (z.view(b, n_head, hs, -1) for z in (q, k, v))
    att = F.softmax((qq * scale) @ kk.transpose(-2, -1), dim=-1)
    return (att @ vv).transpose(2, 3).contiguous().view(b, c, -1)


def softmax_backward(dp, p):
    """dS = P o (dP - rowsum(dP o P)) of S -> softmax(S, -1)."""
    dp, p = _d(dp), _d(p)
    return p * (dp - (dp * p).sum(-1, keepdim=True))


def chan_attn(q, k, v, n_head, scale, grad_out):
    """out (B, C, T) in the ``transpose(2, 3).contiguous().view(B, C, T)`` image, and dq, dk, dv."""
    q, k, v, go = _d(q), _d(k), _d(v), _d(grad_out)
    b, c, t = q.shape
    hs = c // n_head
    qq, kk, vv = (z.reshape(b, n_head, hs, t) for z in (q, k, v))
    s = scale * (qq @ kk.transpose(-2, -1))                               # (B, nh, hs, hs): contraction over T
    s = s - s.max(-1, keepdim=True).values
    p = torch.exp(s)
    p = p / p.sum(-1, keepdim=True)
    o = p @ vv                                                            # (B, nh, hs, T)
    out = o.transpose(2, 3).contiguous().reshape(b, c, t)
    d_o = go.reshape(b, n_head, t, hs).transpose(2, 3)                    # the gradient of o from the (B, nh, T, hs) image
    dv = p.transpose(-2, -1) @ d_o
    ds = softmax_backward(d_o @ vv.transpose(-2, -1), p)
    dq = scale * (ds @ kk)
    dk = scale * (ds.transpose(-2, -1) @ qq)
    return {"out": out, "dq": dq.reshape(b, c, t), "dk": dk.reshape(b, c, t), "dv": dv.reshape(b, c, t)}


def chan_attn_yardstick(q, k, v, n_head, scale, grad_out):
    out, (dq, dk, dv) = _autograd(lambda a, b, c: chan_attn_expr(a, b, c, n_head, scale), [q, k, v], grad_out)
    return {"out": out, "dq": dq, "dk": dk, "dv": dv}


def softmax_backward_padded(slabs, p, hs):
    """otp_softmax_backward: slabs (BH, NS, HSP, HSP), p (BH, HSP, HSP) zero padded beyond hs.  dS of the summed slabs, its
    transpose and the transpose of P, every element of row or column >= hs zero."""
    dp, p = _d(slabs).sum(1), _d(p)
    ds = torch.zeros_like(p)
    ds[:, :hs, :hs] = softmax_backward(dp[:, :hs, :hs], p[:, :hs, :hs])
    pt = torch.zeros_like(p)
    pt[:, :hs, :hs] = p[:, :hs, :hs].transpose(1, 2)
    return {"dS": ds, "dST": ds.transpose(1, 2).contiguous(), "PT": pt}


def softmax_backward_padded_yardstick(slabs, p, hs):
    dp = slabs[:, 0].clone()
    for s in range(1, slabs.shape[1]):
        dp = dp + slabs[:, s]
    ds = torch.zeros_like(p)
    a, b = dp[:, :hs, :hs], p[:, :hs, :hs]
    ds[:, :hs, :hs] = b * (a - (a * b).sum(-1, keepdim=True))
    return {"dS": ds}


# ---- MaxPool1d(3, 2, 1) ----------------------------------------------------------------------------------------------------
def maxpool3s2(x, dy):
    """y and dx of (rows, T): an explicit loop; a window's gradient goes to its FIRST maximum (ties: the lowest index)."""
    x, dy = _d(x), _d(dy)
    rows, t = x.shape
    to = (t + 2 - 3) // 2 + 1
    y, dx = torch.empty(rows, to, dtype=torch.float64), torch.zeros(rows, t, dtype=torch.float64)
    xl, dl = x.tolist(), dy.tolist()
    for r in range(rows):
        for o in range(to):
            best = None
            for i in range(max(0, 2 * o - 1), min(t, 2 * o + 2)):
                if best is None or xl[r][i] > xl[r][best]:
                    best = i
            y[r, o] = xl[r][best]
            dx[r, best] += dl[r][o]
    return {"y": y, "dx": dx}


def maxpool3s2_yardstick(x, dy):
    y, (dx,) = _autograd(lambda a: F.max_pool1d(a.unsqueeze(0), 3, 2, 1).squeeze(0), [x], dy)
    return {"y": y, "dx": dx}


# ---- GELU (exact erf) ------------------------------------------------------------------------------------------------------
def gelu(x, dy):
    x, dy = _d(x), _d(dy)
    cdf = 0.5 * torch.erfc(-x / math.sqrt(2.0))                           # erfc: no cancellation in the negative tail
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return {"y": x * cdf, "dx": dy * (cdf + x * pdf)}


def gelu_yardstick(x, dy):
    y, (dx,) = _autograd(F.gelu, [x], dy)
    return {"y": y, "dx": dx}


# ---- nn.Upsample(scale_factor=f, mode="linear", align_corners=False) on (B, C, T) ------------------------------------------
def upsample_linear_matrix(t, f):
    """(T * f, T) float64: output o reads src = max((o + 0.5) / f - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, T - 1) with
    weights 1 - (src - i0) and src - i0."""
    m = torch.zeros(t * f, t, dtype=torch.float64)
    for o in range(t * f):
        src = max((o + 0.5) / f - 0.5, 0.0)
        i0 = int(src)
        i1 = min(i0 + 1, t - 1)
        m[o, i0] += 1.0 - (src - i0)
        m[o, i1] += src - i0
    return m


def upsample_linear(x, f, dy):
    x, dy = _d(x), _d(dy)
    m = upsample_linear_matrix(x.shape[2], f)
    return {"y": x @ m.t(), "dx": dy @ m}


def upsample_linear_yardstick(x, f, dy):
    if f == 1:                                                            # (torch takes the same path: an identity)
        return {"y": x.clone(), "dx": dy.clone()}
    y, (dx,) = _autograd(lambda a: F.interpolate(a, scale_factor=f, mode="linear", align_corners=False), [x], dy)
    return {"y": y, "dx": dx}


# ---- relu?(res + nearest_upsample_f(low)) of the fuse rows --------------------------------------------------------------------
def nearest_up(low, f):
    return low.repeat_interleave(f, dim=2).repeat_interleave(f, dim=3)


def upsample_add(low, res, f, relu, dy):
    """y, dlow, dres; with the ReLU the gradient passes only where the output is > 0 (an output of exactly 0 passes none)."""
    low, res, dy = _d(low), _d(res), _d(dy)
    n, c, hl, wl = low.shape
    y = res + nearest_up(low, f)
    g = dy
    if relu:
        g = dy * (y > 0).to(torch.float64)
        y = y.clamp_min(0.0)
    return {"y": y, "dres": g, "dlow": g.reshape(n, c, hl, f, wl, f).sum(dim=(3, 5))}


def upsample_add_yardstick(low, res, f, relu, dy):
    def fn(a, b):
        y = b + F.interpolate(a, scale_factor=f, mode="nearest")
        return F.relu(y) if relu else y
    y, (dlow, dres) = _autograd(fn, [low, res], dy)
    return {"y": y, "dres": dres, "dlow": dlow}
