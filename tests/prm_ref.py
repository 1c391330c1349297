"""This project's restatement of RSN_ATTENTION and RSN_WEIGHT_VECTOR (reference model/RSB.py:142-203) in plain torch.  It runs in
whatever dtype its operands have (fp32: the yardstick, fp64: the reference of the GPU tests), in eval mode (running statistics) and
in batch-statistics mode, and is differentiable.  tests/test_prm_host.py holds it against the reference's own classes
(tests/golden/prm.npz).

    cbr(x)      = relu(bn(conv(x)))                                        conv with bias, groups = C for the 9x9
    attention:    f = cbr_prm_1(x);  a = cbr_2_2(cbr_2_1(mean_hw f));  s = cbr_3_2(cbr_3_1(f));  out = f (1 + sigmoid(a) sigmoid(s))
    weight vector: o0 = mean_hw cbr_1(x);  o1 = cbr_2(o0);  out = sigmoid(cbr_3(o1 + o0))

Operator level (folded BatchNorm: per-channel scale and shift): ``prm_gate`` and ``prm_apply`` restate the two inference launches,
``spatial_mean`` / ``dwconv2d`` / ``prm_combine`` the training Functions."""
from __future__ import annotations

import math
import re

import torch
import torch.nn.functional as F

PRM_SEED = 900          # the i-th PRM key (sorted) of a module is drawn with seed PRM_SEED + i
ATT_LAYERS = ("conv_bn_relu_prm_1", "conv_bn_relu_prm_2_1", "conv_bn_relu_prm_2_2", "conv_bn_relu_prm_3_1", "conv_bn_relu_prm_3_2")
VEC_LAYERS = ("conv_bn_relu_1", "conv_bn_relu_2", "conv_bn_relu_3")


# ---- operator level ---------------------------------------------------------------------------------------------------------------
def spatial_mean(x):
    return x.mean(dim=(2, 3), keepdim=True)


def dwconv2d(x, w, bias=None):
    return F.conv2d(x, w, bias, 1, w.shape[-1] // 2, 1, groups=x.shape[1])


def prm_combine(f, a, s):
    return f * (1 + torch.sigmoid(a) * torch.sigmoid(s))


def _affine(z, scale, shift):
    c = z.shape[1]
    return z * scale.reshape(1, c, 1, 1) + shift.reshape(1, c, 1, 1)


def prm_gate(f, w1, scale1, shift1, w2, scale2, shift2, residual=False):
    c = f.shape[1]
    v0 = spatial_mean(f)
    v1 = torch.relu(_affine(F.conv2d(v0, w1.reshape(c, c, 1, 1)), scale1, shift1))
    if residual:
        v1 = v1 + v0
    return torch.sigmoid(torch.relu(_affine(F.conv2d(v1, w2.reshape(c, c, 1, 1)), scale2, shift2)))


def prm_apply(f, gate_c, w31, scale31, shift31, w32, scale32, shift32):
    n, c = f.shape[:2]
    t = torch.relu(_affine(F.conv2d(f, w31.reshape(c, c, 1, 1)), scale31, shift31))
    s = torch.relu(_affine(dwconv2d(t, w32.reshape(c, 1, 9, 9)), scale32, shift32))
    return f * (1 + gate_c.reshape(n, c, 1, 1) * torch.sigmoid(s))


def fold(sd, p, eps=1e-5):
    """(weight, scale, shift) of layer ``p`` in eval mode: BatchNorm and the conv bias as a per-channel scale and shift."""
    sc = sd[p + ".bn.weight"] / torch.sqrt(sd[p + ".bn.running_var"] + eps)
    sh = sd[p + ".bn.bias"] - sd[p + ".bn.running_mean"] * sc + sd[p + ".conv.bias"] * sc
    return sd[p + ".conv.weight"], sc, sh


# ---- module level (state-dict driven) ---------------------------------------------------------------------------------------------
def cbr(sd, p, x, train=False, pre=None, stats=None, eps=1e-5):
    """conv-BN-ReLU of layer ``p``.  ``train``: batch statistics (biased variance), like nn.BatchNorm2d in training mode, which
    refuses one value per channel.  ``pre`` (dict) receives the ReLU's pre-activation, ``stats`` the batch (mean, unbiased var)."""
    w = sd[p + ".conv.weight"]
    z = F.conv2d(x, w, sd[p + ".conv.bias"], 1, w.shape[-1] // 2, 1, groups=x.shape[1] // w.shape[1])
    c = z.shape[1]
    if train:
        count = z.numel() // c
        if count <= 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {list(z.shape)}")
        mean = z.mean(dim=(0, 2, 3))
        var = ((z - mean.reshape(1, c, 1, 1)) ** 2).mean(dim=(0, 2, 3))
        if stats is not None:
            stats[p] = (mean.detach(), var.detach() * count / (count - 1))
    else:
        mean, var = sd[p + ".bn.running_mean"], sd[p + ".bn.running_var"]
    v = (z - mean.reshape(1, c, 1, 1)) / torch.sqrt(var.reshape(1, c, 1, 1) + eps)
    v = v * sd[p + ".bn.weight"].reshape(1, c, 1, 1) + sd[p + ".bn.bias"].reshape(1, c, 1, 1)
    if pre is not None:
        pre[p] = v.detach()
    return torch.relu(v)


def _dot(p, name):
    return f"{p}.{name}" if p else name


def rsn_attention(sd, p, x, train=False, pre=None, stats=None):
    k = dict(train=train, pre=pre, stats=stats)
    f = cbr(sd, _dot(p, ATT_LAYERS[0]), x, **k)
    a = cbr(sd, _dot(p, ATT_LAYERS[2]), cbr(sd, _dot(p, ATT_LAYERS[1]), spatial_mean(f), **k), **k)
    s = cbr(sd, _dot(p, ATT_LAYERS[4]), cbr(sd, _dot(p, ATT_LAYERS[3]), f, **k), **k)
    return prm_combine(f, a, s)


def rsn_weight_vector(sd, p, x, train=False, pre=None, stats=None):
    k = dict(train=train, pre=pre, stats=stats)
    o0 = spatial_mean(cbr(sd, _dot(p, VEC_LAYERS[0]), x, **k))
    o1 = cbr(sd, _dot(p, VEC_LAYERS[1]), o0, **k)
    return torch.sigmoid(cbr(sd, _dot(p, VEC_LAYERS[2]), o1 + o0, **k))


def autograd(fn, leaves, grad_out):
    """(output, gradients) of ``fn(*leaves)`` for the cotangent ``grad_out``."""
    xs = [x.detach().clone().requires_grad_() for x in leaves]
    out = fn(*xs)
    return out.detach(), list(torch.autograd.grad(out, xs, grad_out.to(out.dtype)))


# ---- ReLU kinks -------------------------------------------------------------------------------------------------------------------
KINK_DELTA, KINK_CAP = 1e-5, 0.02


def kink_report(pre):
    """{layer: (share of pre-activations within KINK_DELTA of zero, is a gate-vector layer)} of the ``pre`` dict of a float64 run.
    A ReLU whose pre-activation is that close to zero may open in one precision and close in the other; the gradient tests may
    leave such elements out - at most KINK_CAP of a tensor, and none on the (N, C, 1, 1) gate vectors, each value of which steers
    a whole channel."""
    return {p: (float((v.abs() < KINK_DELTA).double().mean()), v.shape[2] * v.shape[3] == 1) for p, v in pre.items()}


def kink_pixels(pre, shape):
    """(N, 1, H, W) bool: pixels at which a full-resolution pre-activation of ``pre`` is within KINK_DELTA of zero in any channel."""
    near = torch.zeros((shape[0], 1, shape[2], shape[3]), dtype=torch.bool)
    for v in pre.values():
        if tuple(v.shape[2:]) == tuple(shape[2:]):
            near |= (v.abs() < KINK_DELTA).any(dim=1, keepdim=True)
    return near


# ---- weights: a seeded rule for the PRM keys, the synthetic recipe for every other key ---------------------------------------------
def is_prm_key(k):
    return "conv_bn_relu_prm_" in k or re.search(r"(^|\.)conv_bn_relu_[123]\.", k) is not None


def prm_values(shapes):
    """{key: tensor} for the PRM keys of ``shapes`` ({key: shape}), key i (sorted) from seed PRM_SEED + i: conv weights
    N(0, 2 / fan_in), conv biases N(0, 0.05^2), BatchNorm weights 1 + N(0, 0.1^2), biases and running means N(0, 0.1^2), running
    variances U(0.8, 1.2); ``num_batches_tracked`` keeps its constructor value."""
    out = {}
    for i, k in enumerate(sorted(k for k in shapes if is_prm_key(k))):
        shape = tuple(shapes[k])
        leaf = k.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            continue
        g = torch.Generator().manual_seed(PRM_SEED + i)
        if leaf == "running_var":
            out[k] = 0.8 + 0.4 * torch.rand(shape, generator=g)
            continue
        r = torch.randn(shape, generator=g, dtype=torch.float32)
        if len(shape) == 4:
            out[k] = r * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        elif ".bn." in k:
            out[k] = 1.0 + 0.1 * r if leaf == "weight" else 0.1 * r
        else:
            out[k] = 0.05 * r
    return out


def prm_state(shapes, seed, gains=None):
    """Values for a whole key set: ``synthetic.synthetic_state_dict`` sees the keys WITHOUT the PRM ones (so it draws exactly
    what it draws for the model without them), the PRM keys follow :func:`prm_values`."""
    from otpose_amd import synthetic as S
    rest = {k: s for k, s in shapes.items() if not is_prm_key(k)}
    new = S.synthetic_state_dict(rest, seed, gains) if rest else {}
    new.update(prm_values(shapes))
    return new


def fill_prm_(module, seed, gains=None):
    """``synthetic.fill_synthetic_`` for a module with PRM keys (an OTPose with ``MODEL.PRM``, or a bare RSN_* module)."""
    from otpose_amd import synthetic as S
    sd = module.state_dict()
    if gains is None and getattr(module, "cfg", None) is not None:
        gains = S.gains_for(module.cfg)
    new = prm_state({k: tuple(v.shape) for k, v in sd.items()}, seed, gains)
    with torch.no_grad():
        for k, v in new.items():
            sd[k].copy_(v.to(sd[k].dtype))
    return module
