"""This project's restatement of the token x token attention of the DETR-style TransformerEncoder (reference model/OTPose.py:26-159,
259-305) in plain torch, with an explicit T x T softmax.  It runs in whatever dtype its operands have (fp32: the yardstick, fp64:
the reference of the GPU tests) and is differentiable.

    S[b,h,i,j] = scale * sum_c q[b,h,c,i] k[b,h,c,j]   (-inf where key j of sample b is padding)
    P = softmax_j(S),   O[b, h*hd+c, i] = sum_j P[b,h,i,j] v[b,h,c,j]

Module level (state-dict driven): ``encoder_layer`` / ``encoder`` on sequence-first (L, N, E) tensors, eval mode.
tests/test_token_attn_host.py holds these against the reference's own classes (tests/golden/token_encoder.npz)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

FILL_SEED = 700          # the i-th key (sorted) of a module is drawn with seed FILL_SEED + seed + i


def token_attn_probs(q, k, nh, scale, mask=None):
    """(B, nh, T, T) softmax weights; ``mask`` (B, T) bool, True = padding."""
    b, c, t = q.shape
    hd = c // nh
    s = torch.einsum("bhci,bhcj->bhij", q.reshape(b, nh, hd, t), k.reshape(b, nh, hd, t)) * scale
    if mask is not None:
        s = s.masked_fill(mask.reshape(b, 1, 1, t), float("-inf"))
    return F.softmax(s, dim=-1)


def token_attn(q, k, v, nh, scale, mask=None):
    """q, k, v (B, C, T) -> (B, C, T)."""
    b, c, t = q.shape
    p = token_attn_probs(q, k, nh, scale, mask)
    return torch.einsum("bhij,bhcj->bhci", p, v.reshape(b, nh, c // nh, t)).reshape(b, c, t)


def token_attn_map(q, k, nh, scale, mask=None):
    """(B, T, T): the mean over heads of P."""
    return token_attn_probs(q, k, nh, scale, mask).mean(dim=1)


def autograd(fn, leaves, grad_out):
    """(output, gradients) of ``fn(*leaves)`` for the cotangent ``grad_out``; a None leaf gets a None gradient."""
    xs = [None if x is None else x.detach().clone().requires_grad_() for x in leaves]
    out = fn(*xs)
    live = [x for x in xs if x is not None]
    grads = iter(torch.autograd.grad(out, live, grad_out.to(out.dtype)))
    return out.detach(), [None if x is None else next(grads) for x in xs]


def sine_table(h, w, d_model, temperature=10000, scale=2 * math.pi, dtype=torch.float32):
    """(1, h w, d_model): per token (row y, column x), features [row half | column half], each half sin / cos interleaved over
    the wavelengths temperature^(2 (i // 2) / (d_model / 2)) of the position normalised to (0, scale]."""
    half = d_model // 2
    i = torch.arange(half, dtype=dtype)
    wave = temperature ** (2 * torch.div(i, 2, rounding_mode="floor") / half)
    even = (torch.arange(half) % 2 == 0)

    def enc(n):
        pos = torch.arange(1, n + 1, dtype=dtype) / (n + 1e-6) * scale
        ang = pos[:, None] / wave[None, :]
        return torch.where(even[None, :], ang.sin(), ang.cos())

    ey, ex = enc(h), enc(w)
    return torch.cat((ey[:, None, :].expand(h, w, half), ex[None, :, :].expand(h, w, half)), dim=2).reshape(1, h * w, d_model)


# ---- module level ------------------------------------------------------------------------------------------------------------------
def _ln(sd, p, x):
    return F.layer_norm(x, x.shape[-1:], sd[p + ".weight"], sd[p + ".bias"], 1e-5)


def _self_attn(sd, p, qk, value, nh, mask):
    """nn.MultiheadAttention(E, nh) in eval mode on (L, N, E): in-projection, the attention above, out-projection."""
    e = qk.shape[-1]
    w, b = sd[p + ".in_proj_weight"], sd[p + ".in_proj_bias"]
    q = F.linear(qk, w[:e], b[:e]).permute(1, 2, 0)                # (N, E, L): the library's layout
    k = F.linear(qk, w[e:2 * e], b[e:2 * e]).permute(1, 2, 0)
    v = F.linear(value, w[2 * e:], b[2 * e:]).permute(1, 2, 0)
    scale = 1.0 / math.sqrt(e // nh)
    o = token_attn(q, k, v, nh, scale, mask).permute(2, 0, 1)
    return F.linear(o, sd[p + ".out_proj.weight"], sd[p + ".out_proj.bias"]), token_attn_map(q, k, nh, scale, mask)


def encoder_layer(sd, p, src, nh, activation, pre_norm, mask=None, pos=None):
    """TransformerEncoderLayer.forward_post / forward_pre in eval mode; returns (output, attention map)."""
    act = {"relu": F.relu, "gelu": F.gelu}[activation]
    ffn = lambda x: F.linear(act(F.linear(x, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"])),     # noqa: E731
                             sd[p + ".linear2.weight"], sd[p + ".linear2.bias"])
    if pre_norm:
        x = _ln(sd, p + ".norm1", src)
        a, amap = _self_attn(sd, p + ".self_attn", x if pos is None else x + pos, src, nh, mask)
        src = src + a
        return src + ffn(_ln(sd, p + ".norm2", src)), amap
    a, amap = _self_attn(sd, p + ".self_attn", src if pos is None else src + pos, src, nh, mask)
    src = _ln(sd, p + ".norm1", src + a)
    return _ln(sd, p + ".norm2", src + ffn(src)), amap


def encoder(sd, src, num_layers, nh, activation, pre_norm, mask=None, pos=None, pe_only_at_begin=False):
    """TransformerEncoder.forward in eval mode: (output, (layers, N, L, L) attention maps); ``norm.*`` is applied when present."""
    maps = []
    for i in range(num_layers):
        src, amap = encoder_layer(sd, f"layers.{i}", src, nh, activation, pre_norm, mask, pos)
        maps.append(amap)
        if pe_only_at_begin:
            pos = None
    if "norm.weight" in sd:
        src = _ln(sd, "norm", src)
    return src, torch.stack(maps)


# ---- weights: a seeded fill shared by the fixture generator and the tests ----------------------------------------------------------
def encoder_values(shapes, seed):
    """{key: tensor} for a key set ({key: shape}), key i (sorted) from seed FILL_SEED + seed + i: matrices N(0, 1 / fan_in),
    LayerNorm weights 1 + N(0, 0.1^2), every other vector N(0, 0.1^2)."""
    out = {}
    for i, k in enumerate(sorted(shapes)):
        shape = tuple(shapes[k])
        r = torch.randn(shape, generator=torch.Generator().manual_seed(FILL_SEED + seed + i), dtype=torch.float32)
        if len(shape) == 2:
            out[k] = r / math.sqrt(shape[1])
        elif "norm" in k and k.endswith("weight"):
            out[k] = 1.0 + 0.1 * r
        else:
            out[k] = 0.1 * r
    return out


def fill_encoder_(module, seed):
    sd = module.state_dict()
    with torch.no_grad():
        for k, v in encoder_values({k: tuple(v.shape) for k, v in sd.items()}, seed).items():
            sd[k].copy_(v)
    return module
