"""This project's restatement of the attention-probability dropout (include/otpose_hip.h, "attention dropout mask"): the mask in
numpy uint32 / uint64 arithmetic, and the three attentions in plain torch taking an explicit mask.  The attentions are built on
the restatements the undropped kernels are held against - tests/token_attn_ref.py, tests/local_attn_ref.py and the channel
attention of tests/encoder_bwd_ref.py - run in whatever dtype their operands have (fp64: the reference of the GPU tests, fp32:
the yardstick) and are differentiable.

    thr  = (uint32)(p * 65536.f + 0.5f)
    pair = ((uint64)g * R + i) * ((Ccols + 1) / 2) + (j >> 1)
    h    = hash(pair, seed)                       two 16-bit uniforms per hash
    keep = ((j & 1) ? h >> 16 : h & 0xFFFF) >= thr;    survivors are multiplied by 65536.f / (65536 - thr)

The softmax is the undropped one; only the operand of the P v product is multiplied by the mask."""
from __future__ import annotations

import numpy as np
import torch

from tests import encoder_bwd_ref as E
from tests import local_attn_ref as LR
from tests import token_attn_ref as TR

U32 = np.uint32
M32 = np.uint64(0xFFFFFFFF)


def threshold(p):
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def keep_scale(p):
    """What a survivor is multiplied by, as the float32 value the kernels use."""
    thr = threshold(p)
    return float(np.float32(65536.0) / np.float32(65536 - thr)) if thr < 65536 else 0.0


def drop_hash(pair, seed):
    """``otp_drop_hash`` on a uint64 array of pair indices: every step wraps at 32 bits."""
    pair = np.asarray(pair, dtype=np.uint64)
    s0, s1 = U32(seed & 0xFFFFFFFF), U32((seed >> 32) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        h = (pair & M32).astype(U32) * U32(0x9E3779B1) + s0
        h ^= ((pair >> np.uint64(32)).astype(U32) + s1) * U32(0x85EBCA77)
        h ^= h >> U32(16)
        h *= U32(0x21F0AAAD)
        h ^= h >> U32(15)
        h *= U32(0x735A2D97)
        h ^= h >> U32(15)
    return h


def keep(seed, G, R, Ccols, p):
    """(G, R, Ccols) bool numpy array, True = kept."""
    thr = U32(threshold(p))
    half = (Ccols + 1) // 2
    with np.errstate(over="ignore"):
        row = np.arange(G * R, dtype=np.uint64).reshape(G, R, 1) * np.uint64(half)
        h = drop_hash(row + np.arange(half, dtype=np.uint64).reshape(1, 1, half), seed)            # (G, R, half)
    u16 = np.stack((h & U32(0xFFFF), h >> U32(16)), axis=-1).reshape(G, R, 2 * half)[:, :, :Ccols]
    return u16 >= thr


def factors(seed, G, R, Ccols, p, dtype=torch.float64):
    """(G, R, Ccols) tensor: ``keep_scale(p)`` for a survivor, 0 for a dropped entry."""
    return torch.from_numpy(keep(seed, G, R, Ccols, p)).to(dtype) * keep_scale(p)


# ---- the three attentions with an explicit factor tensor m (G = B * n_head first) -------------------------------------------------
def token_attn(q, k, v, nh, scale, m, mask=None):
    """tests/token_attn_ref.token_attn with P m in front of the second product; ``m`` (B * nh, T, T)."""
    b, c, t = q.shape
    p = TR.token_attn_probs(q, k, nh, scale, mask) * m.reshape(b, nh, t, t).to(q.dtype)
    return torch.einsum("bhij,bhcj->bhci", p, v.reshape(b, nh, c // nh, t)).reshape(b, c, t)


def local_attn(q, k, v, nh, window, scale, m, rel_pe=None):
    """tests/local_attn_ref.local_attn with P m; ``m`` (B * nh, T, window)."""
    b, c, t = q.shape
    p = LR.local_attn_probs(q, k, nh, window, scale, rel_pe) * m.reshape(b, nh, t, window).to(q.dtype)
    idx, _ = LR.band_index(t, window, q.device)
    return torch.einsum("bhtj,bhctj->bhct", p, v.reshape(b, nh, c // nh, t)[..., idx]).reshape(b, c, t)


def chan_attn(q, k, v, nh, scale, m):
    """tests/encoder_bwd_ref.chan_attn_expr with P m; ``m`` (B * nh, hs, hs).  Result in the transposed-contiguous image."""
    b, c, _ = q.shape
    hs = c // nh
    qq, kk, vv = (z.view(b, nh, hs, -1) for z in (q, k, v))
    att = torch.softmax((qq * scale) @ kk.transpose(-2, -1), dim=-1) * m.reshape(b, nh, hs, hs).to(q.dtype)
    return (att @ vv).transpose(2, 3).contiguous().view(b, c, -1)


def ones(G, R, Ccols, dtype=torch.float64):
    return torch.ones(G, R, Ccols, dtype=dtype)


autograd = TR.autograd
chan_attn_expr = E.chan_attn_expr
