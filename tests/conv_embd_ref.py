"""This project's restatement of the conv embedding of ConvTransformer (reference model/ConvVideoTransformer.py:60-78, 129-135)
in plain torch; it runs in whatever dtype its operands have (fp32: the yardstick, fp64: the reference of the GPU tests) and is
differentiable.

    z = conv2d(x, weight, bias, stride 1, padding ks // 2)                     x (B, Cin, H, W), zero padding
    v = z.flatten(2);  with a norm: v = (v - mean_c v) / sqrt(mean_c (v - mean_c v)^2 + eps) * ln_weight + ln_bias
    y = relu(v) (+ pe)                                                         (B, Cout, H W)

Module level (state-dict driven, like oracle/otpose_oracle.py): ``conv_transformer`` runs the ``arch[0]`` embedding layers, adds
the positional table and continues with the oracle's blocks.  tests/test_conv_embd_host.py holds it against the reference's own
classes (tests/golden/conv_embd.npz)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import otpose_oracle as O

EMBD_SEED = 700         # the i-th conv embedding key (sorted) of a module is drawn with seed EMBD_SEED + i


def pre_activation(x, weight, bias, ln_weight, ln_bias, eps=1e-5):
    """What the ReLU sees, (B, Cout, H W)."""
    ks = weight.shape[-1]
    v = F.conv2d(x, weight, bias, 1, ks // 2).flatten(2)
    if ln_weight is not None:
        c = v.shape[1]
        res = v - v.mean(dim=1, keepdim=True)
        sigma = (res ** 2).mean(dim=1, keepdim=True)
        v = res / torch.sqrt(sigma + eps) * ln_weight.reshape(1, c, 1) + ln_bias.reshape(1, c, 1)
    return v


def conv_embd(x, weight, bias, ln_weight, ln_bias, pe=None, eps=1e-5):
    y = F.relu(pre_activation(x, weight, bias, ln_weight, ln_bias, eps))
    return y if pe is None else y + pe.reshape(1, y.shape[1], y.shape[2])


def autograd(fn, leaves, grad_out):
    """(output, gradients) of ``fn(*leaves)`` for the cotangent ``grad_out``; a None leaf gets a None gradient."""
    xs = [None if x is None else x.detach().clone().requires_grad_() for x in leaves]
    out = fn(*xs)
    live = [x for x in xs if x is not None]
    grads = iter(torch.autograd.grad(out, live, grad_out.to(out.dtype)))
    return out.detach(), [None if x is None else next(grads) for x in xs]


# ---- module level ----------------------------------------------------------------------------------------------------------------
def embed(sd, p, x4):
    """The embedding layers of encoder ``p`` on x4 (B, n_in, H, W) -> (B, n_embd, H, W); none: x4 itself."""
    b, _, h, w = x4.shape
    i = 0
    while f"{p}.embd.{i}.weight" in sd:
        y = conv_embd(x4, sd[f"{p}.embd.{i}.weight"], sd.get(f"{p}.embd.{i}.bias"), sd.get(f"{p}.embd_norm.{i}.weight"),
                      sd.get(f"{p}.embd_norm.{i}.bias"))
        x4 = y.reshape(b, -1, h, w)
        i += 1
    return x4


def conv_transformer(sd, p, x4, n_head, arch):
    """ConvVideoTransformer.py:123-184 in eval mode (channel attention; T <= max_len).  A block built with path_pdrop = 0 has
    no AffineDropPath (blocks.py:256-262: the residual is added as it is): the oracle's block then sees a scale of one."""
    x4 = embed(sd, p, x4)
    b, c, h, w = x4.shape
    sd = dict(sd)
    for i, kind in [(i, "stem") for i in range(arch[1])] + [(i, "branch") for i in range(arch[2])]:
        for name in ("drop_path_attn", "drop_path_mlp"):
            sd.setdefault(f"{p}.{kind}.{i}.{name}.scale", torch.ones(1, c, 1, dtype=x4.dtype))
    t = h * w
    x = x4.reshape(b, c, t) + sd[p + ".pos_embd"][:, :, :t]
    for i in range(arch[1]):
        x = O.transformer_block(sd, f"{p}.stem.{i}", x, n_head, 1)
    outs = [x]
    for i in range(arch[2]):
        x = O.transformer_block(sd, f"{p}.branch.{i}", x, n_head, 2)
        outs.append(F.interpolate(x, scale_factor=2 ** (i + 1), mode="linear", align_corners=False))
    return outs


# ---- weights of a module with embedding layers: the synthetic recipe for every other key, a seeded rule for the new ones ------------
def is_embd_key(k):
    return ".embd." in f".{k}" or ".embd_norm." in f".{k}"


def embd_values(shapes):
    """{key: tensor} for the conv embedding keys of ``shapes`` ({key: shape}): conv weights N(0, 2 / fan_in), conv biases
    N(0, 0.05^2), norm weights 1 + N(0, 0.1^2), norm biases N(0, 0.1^2), key i (sorted) from seed EMBD_SEED + i."""
    out = {}
    for i, k in enumerate(sorted(k for k in shapes if is_embd_key(k))):
        shape = tuple(shapes[k])
        g = torch.Generator().manual_seed(EMBD_SEED + i)
        r = torch.randn(shape, generator=g, dtype=torch.float32)
        leaf = k.rsplit(".", 1)[-1]
        if len(shape) == 4:
            out[k] = r * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        elif ".embd_norm." in f".{k}":
            out[k] = 1.0 + 0.1 * r if leaf == "weight" else 0.1 * r
        else:
            out[k] = 0.05 * r
    return out


def fill_embd_(module, seed, gains=None):
    """``synthetic.fill_synthetic_`` for a module with conv embedding layers: the recipe sees the key set WITHOUT them (so it
    draws exactly what it draws for the module without an embedding), the new keys follow :func:`embd_values`."""
    from otpose_amd import synthetic as S
    sd = module.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    if gains is None and getattr(module, "cfg", None) is not None:
        gains = S.gains_for(module.cfg)
    new = S.synthetic_state_dict({k: s for k, s in shapes.items() if not is_embd_key(k)}, seed, gains)
    new.update(embd_values(shapes))
    with torch.no_grad():
        for k, v in new.items():
            sd[k].copy_(v.to(sd[k].dtype))
    return module
