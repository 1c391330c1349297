"""Token x token self-attention on the GPU (csrc/tokattn.hip): the attention core of the DETR-style ``TransformerEncoder`` of the
reference's model/OTPose.py:26-159, flash style - online softmax over key tiles, a recomputing backward, no T x T buffer.

Operands are the library's own layout: ``q, k, v`` fp32 ``(B, C, T)``, contiguous, head ``h`` owning channels
``h * hd .. (h + 1) * hd - 1`` (``nn.MultiheadAttention``'s head split with the token axis last):

    S[i][j] = scale * sum_c q[c][i] k[c][j],   P = softmax_j(S),   O[c][i] = sum_j P[i][j] v[c][j]

``key_padding_mask`` is ``(B, T)`` bool, True = this key is padding, as in PyTorch.  A sample whose keys are all padding is
outside the contract (PyTorch returns NaN rows there; this kernel divides by zero).  ``dropout_p`` > 0 drops attention
probabilities inside the kernels (the mask of otpose_amd/attn_dropout.py: the softmax statistics stay undropped, only the operand
of the P v product is masked and scaled by 1 / (1 - p)); the backward re-evaluates the same mask from the seed.  Supported: ``C % n_head == 0`` and a head
width of at most 136; everything else raises ``ValueError`` before any launch.  CPU tensors raise ``NotImplementedError``,
like every operator here.

``products="half"`` (``token_attn`` only) runs the half-operand kernels of csrc/tokattn_h.hip: ``scale q``, ``k``, ``v``, the
incoming gradient and the probabilities are rounded to IEEE half on their way into the 16-bit matrix cores, every sum, the softmax
and every tensor in memory stay fp32.  Its operands must stay below 65504 in magnitude (:func:`check_range`).
"""
from __future__ import annotations

import math

import torch
from torch.autograd import Function

from . import attn_dropout, hip
from .ops import require_gpu

__all__ = ["token_attn", "token_attn_map", "sine_position_embedding", "check_token_attn", "check_products", "check_range",
           "MAX_HEAD_WIDTH", "PRODUCTS"]

MAX_HEAD_WIDTH = 136
PRODUCTS = ("f32", "half")


def check_products(products, what="token_attn: products"):
    """Raise ``ValueError`` unless ``products`` names an arithmetic mode of the token attention; returns it."""
    if not isinstance(products, str) or products not in PRODUCTS:
        raise ValueError(f"{what} must be one of {PRODUCTS}, got {products!r}")
    return products


def check_token_attn(c, n_head, t):
    """Raise ``ValueError`` for a shape the kernels do not take (``otp_token_attn_supported``)."""
    if not isinstance(n_head, int) or isinstance(n_head, bool) or n_head <= 0 or c % n_head:
        raise ValueError(f"token_attn: {c} channels do not split into {n_head!r} heads")
    if not hip.lib().otp_token_attn_supported(int(c), n_head, int(t)):
        raise ValueError(f"token_attn: the head width C / n_head must be in [1, {MAX_HEAD_WIDTH}] and T at least 1, got C = {c}, "
                         f"n_head = {n_head}, T = {t}")


def _check(q, k, v, n_head, key_padding_mask):
    """Validate the operands and return (B, C, T, mask as uint8 or None)."""
    tensors = [x for x in (q, k, v) if x is not None]
    for x in tensors:
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError("token_attn: q, k, v are (B, C, T) tensors")
        if x.dtype != torch.float32:
            raise ValueError(f"token_attn: built for float32, got {x.dtype}")
        if not x.is_contiguous():
            raise ValueError("token_attn: q, k, v must be contiguous (B, C, T) tensors")
        if x.shape != q.shape or x.device != q.device:
            raise ValueError(f"token_attn: operands of different shapes or devices: {tuple(x.shape)} and {tuple(q.shape)}")
    b, c, t = q.shape
    if b < 1:
        raise ValueError("token_attn: an empty batch")
    check_token_attn(c, n_head, t)
    mask = None
    if key_padding_mask is not None:
        if not isinstance(key_padding_mask, torch.Tensor) or key_padding_mask.dtype != torch.bool:
            raise ValueError("token_attn: key_padding_mask is a bool tensor (True = padding)")
        if tuple(key_padding_mask.shape) != (b, t) or key_padding_mask.device != q.device:
            raise ValueError(f"token_attn: key_padding_mask must be ({b}, {t}) on the operands' device, got "
                             f"{tuple(key_padding_mask.shape)}")
        mask = key_padding_mask.contiguous().view(torch.uint8)
    require_gpu(*tensors)
    return b, c, t, mask


def _forward(q, k, v, mask, n_head, scale, want_lse, p=0.0, seed=0):
    b, c, t = q.shape
    out = torch.empty_like(q)
    lse = torch.empty((b, n_head, t), dtype=torch.float32, device=q.device) if want_lse else None
    if p > 0.0:
        hip.check(hip.lib().otp_token_attn_forward_dropout(hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(mask), hip.ptr(out),
                                                           hip.ptr(lse), b, c, n_head, t, scale, p, seed, hip.stream_of(q)),
                  "otp_token_attn_forward_dropout")
        return out, lse
    hip.check(hip.lib().otp_token_attn_forward(hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(mask), hip.ptr(out), hip.ptr(lse),
                                               b, c, n_head, t, scale, hip.stream_of(q)), "otp_token_attn_forward")
    return out, lse


class TokenAttnFunction(Function):
    """``token_attn`` with a backward: the forward keeps q, k, v, the output and the row log-sum-exp (B, n_head, T); the backward
    is ``otp_token_attn_backward`` (pass A: D and dq per query tile, pass B: dk and dv per key tile; deterministic, no atomics).
    With ``p`` > 0 both directions run the ``_dropout`` entry points under the same ``seed``: no mask is stored."""

    @staticmethod
    def forward(ctx, q, k, v, mask, n_head, scale, p=0.0, seed=0):
        out, lse = _forward(q, k, v, mask, n_head, scale, True, p, seed)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.mask, ctx.cfg, ctx.drop = mask, (n_head, scale), (p, seed)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, out, lse = ctx.saved_tensors
        n_head, scale = ctx.cfg
        b, c, t = q.shape
        L = hip.lib()
        gout = gout.contiguous()
        gq, gk, gv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        ws = torch.empty(L.otp_token_attn_workspace(b, n_head, t, c // n_head) // 4, dtype=torch.float32, device=q.device)
        p, seed = ctx.drop
        if p > 0.0:
            hip.check(L.otp_token_attn_backward_dropout(hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(ctx.mask), hip.ptr(out),
                                                        hip.ptr(lse), hip.ptr(gout), hip.ptr(gq), hip.ptr(gk), hip.ptr(gv),
                                                        hip.ptr(ws), b, c, n_head, t, scale, p, seed, hip.stream_of(q)),
                      "otp_token_attn_backward_dropout")
            return gq, gk, gv, None, None, None, None, None
        hip.check(L.otp_token_attn_backward(hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(ctx.mask), hip.ptr(out), hip.ptr(lse),
                                            hip.ptr(gout), hip.ptr(gq), hip.ptr(gk), hip.ptr(gv), hip.ptr(ws), b, c, n_head, t,
                                            scale, hip.stream_of(q)), "otp_token_attn_backward")
        return gq, gk, gv, None, None, None, None, None


def check_range(device=None):
    """The host side of the half kernels' range guard (csrc/range.hip): synchronise ``device`` and raise ``FloatingPointError`` if
    a 16-bit-operand kernel of this process has seen a value beyond a half's range since the last check; the sticky word is
    cleared.  ``token_attn(products="half")`` calls it after every eager launch; under a stream capture it cannot (the tensors
    of a violating launch are NaN-filled on the device all the same) and the owner of the graph calls it after a replay."""
    torch.cuda.synchronize(device)
    code = hip.lib().otp_range_flag_read(1)
    if code:
        raise FloatingPointError(
            f"otpose_amd.token_attn: a value left the range of an IEEE half (|x| >= 65504, or a non-finite sum; kernel family "
            f"{code}, 12 = token attention with half products); the tensors of that launch were NaN-filled on the device.  "
            "Rescale the operands or use products='f32'.")


def _guard(device, *outs):
    """Behind a launch of the half kernels: NaN into ``outs`` on the device if the guard word is set, then the host check."""
    for t in outs:
        if t is not None:
            hip.check(hip.lib().otp_range_poison(hip.ptr(t), t.numel(), hip.stream_of(t)), "otp_range_poison")
    if not torch.cuda.is_current_stream_capturing():
        check_range(device)


def _forward_half(q, k, v, mask, n_head, scale, want_lse, p=0.0, seed=0):
    b, c, t = q.shape
    out = torch.empty_like(q)
    lse = torch.empty((b, n_head, t), dtype=torch.float32, device=q.device) if want_lse else None
    hip.check(hip.lib().otp_token_attn_forward_h1(hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(mask), hip.ptr(out), hip.ptr(lse),
                                                  b, c, n_head, t, scale, p, seed, None, hip.stream_of(q)),
              "otp_token_attn_forward_h1")
    _guard(q.device, out)
    return out, lse


class TokenAttnHalfFunction(Function):
    """``token_attn(products="half")`` with a backward: ``otp_token_attn_forward_h1`` / ``otp_token_attn_backward_h1``, which keep
    what :class:`TokenAttnFunction` keeps.  The gradient is that of the rounded forward with the roundings passed straight
    through; the backward rounds its own operands (``dout``, dS) to half as well."""

    @staticmethod
    def forward(ctx, q, k, v, mask, n_head, scale, p=0.0, seed=0):
        out, lse = _forward_half(q, k, v, mask, n_head, scale, True, p, seed)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.mask, ctx.cfg, ctx.drop = mask, (n_head, scale), (p, seed)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, out, lse = ctx.saved_tensors
        n_head, scale = ctx.cfg
        b, c, t = q.shape
        L = hip.lib()
        gout = gout.contiguous()
        gq, gk, gv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        ws = torch.empty(L.otp_token_attn_h1_workspace(b, n_head, t, c // n_head) // 4, dtype=torch.float32, device=q.device)
        p, seed = ctx.drop
        hip.check(L.otp_token_attn_backward_h1(hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(ctx.mask), hip.ptr(out), hip.ptr(lse),
                                               hip.ptr(gout), hip.ptr(gq), hip.ptr(gk), hip.ptr(gv), hip.ptr(ws), b, c, n_head, t,
                                               scale, p, seed, None, hip.stream_of(q)), "otp_token_attn_backward_h1")
        _guard(q.device, gq, gk, gv)
        return gq, gk, gv, None, None, None, None, None


def token_attn(q, k, v, n_head, scale, key_padding_mask=None, dropout_p=0.0, seed=None, products="f32"):
    """softmax(scale q^T k) v per head, ``(B, C, T)`` in and out.  Under ``torch.no_grad()`` or with no operand requiring a
    gradient: one forward launch that stores no log-sum-exp; otherwise an autograd Function.

    ``dropout_p`` in [0, 1) (``ValueError`` otherwise) drops attention probabilities: every P[i][j] is zeroed with probability
    ``dropout_p`` and the survivors are scaled by 1 / (1 - dropout_p) in front of the P v product, as ``nn.MultiheadAttention``
    does in training.  ``seed`` (an int below 2^64) fixes the mask; None draws one per call from PyTorch's CUDA generator, so
    ``torch.manual_seed`` makes it repeat.  A rate whose 16-bit threshold is 0 (below 2^-17) is the call without dropout,
    bit for bit, and draws nothing.  Under ``no_grad`` the dropout still applies: forward only.

    ``products``: ``"f32"`` (default) multiplies on the exact-fp32 matrix instruction; ``"half"`` rounds ``scale q``, ``k``,
    ``v``, the incoming gradient and the probabilities to IEEE half in front of the 16-bit matrix cores and accumulates in fp32
    (csrc/tokattn_h.hip) - same operands, same mask and dropout semantics, outputs and gradients to about 2^-11 of their range.
    There an operand of magnitude 65504 or more raises ``FloatingPointError`` and leaves the result NaN-filled
    (:func:`check_range`; eager calls synchronise for it).  Anything else raises ``ValueError`` before any launch."""
    check_products(products)
    p = attn_dropout.check_rate(dropout_p, "token_attn: dropout_p")
    _, _, _, mask = _check(q, k, v, n_head, key_padding_mask)
    scale = float(scale)
    p, seed = attn_dropout.seed_of(p, seed, q.device)
    half = products == "half"
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        return (TokenAttnHalfFunction if half else TokenAttnFunction).apply(q, k, v, mask, n_head, scale, p, seed)
    return (_forward_half if half else _forward)(q, k, v, mask, n_head, scale, False, p, seed)[0]


def token_attn_map(q, k, n_head, scale, key_padding_mask=None):
    """``(B, T, T)``: the mean over heads of P, what ``nn.MultiheadAttention`` returns as its second value.  Two launches: a
    forward for the row log-sum-exp (its output is dropped), then one pass that recomputes ``exp(S - lse)``.

    The map carries NO gradient (a documented deviation: in PyTorch the averaged weights are differentiable), and it is the
    map of the UNDROPPED probabilities (a second deviation: in training ``nn.MultiheadAttention`` returns the weights after its
    dropout; ``token_attn``'s ``dropout_p`` does not reach this function)."""
    b, c, t, mask = _check(q, k, None, n_head, key_padding_mask)
    scale = float(scale)
    q, k = q.detach(), k.detach()
    _, lse = _forward(q, k, k, mask, n_head, scale, True)
    out = torch.empty((b, t, t), dtype=torch.float32, device=q.device)
    hip.check(hip.lib().otp_token_attn_map(hip.ptr(q), hip.ptr(k), hip.ptr(mask), hip.ptr(lse), hip.ptr(out), b, c, n_head, t,
                                           scale, hip.stream_of(q)), "otp_token_attn_map")
    return out


def sine_position_embedding(h, w, d_model, temperature=10000, scale=2 * math.pi):
    """The fixed 2-D sine table of ``_make_sine_position_embedding`` (OTPose.py:281-305) for an ``h x w`` token grid:
    ``(1, h * w, d_model)``, the first half of the width encoding the row, the second half the column, each as interleaved
    sin / cos pairs of the normalised position over a geometric ladder of wavelengths.  ``d_model`` must be a multiple of 4
    (each direction needs whole sin / cos pairs; the reference's own stack / cat fails or yields another width otherwise)."""
    if not isinstance(d_model, int) or d_model <= 0 or d_model % 4:
        raise ValueError(f"sine_position_embedding: d_model must be a positive multiple of 4, got {d_model!r}")
    if h < 1 or w < 1:
        raise ValueError(f"sine_position_embedding: an empty {h} x {w} grid")
    half = d_model // 2
    rows = torch.arange(1, h + 1, dtype=torch.float32) / (h + 1e-6) * scale
    cols = torch.arange(1, w + 1, dtype=torch.float32) / (w + 1e-6) * scale
    ladder = torch.arange(half, dtype=torch.float32)
    ladder = temperature ** (2 * torch.div(ladder, 2, rounding_mode="floor") / half)

    def direction(coord):                                          # (n) -> (n, half): sin on even, cos on odd features
        ang = coord[:, None] / ladder
        return torch.stack((ang[:, 0::2].sin(), ang[:, 1::2].cos()), dim=2).flatten(1)

    py = direction(rows)[:, None, :].expand(h, w, half)
    px = direction(cols)[None, :, :].expand(h, w, half)
    return torch.cat((py, px), dim=2).reshape(1, h * w, d_model).contiguous()
