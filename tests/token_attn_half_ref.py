"""The rounded restatement of the token attention with half products (csrc/tokattn_h.hip) in plain torch: tests/token_attn_ref.py
with ``scale q``, ``k``, ``v`` and the unnormalised probabilities rounded to IEEE half and back where the kernel converts them.

    S = h(scale q)^T h(k)   (-inf at padding),   E = exp(S - M),   W = exp(M - max_j S),   O = (sum_j h(f E) W h(v)) / sum_j E W

``f`` is the dropout factor (1 without dropout).  ``M[i][j]`` is the kernel's running maximum: the largest score of query i over
the 64-key tiles up to and including key j's (online softmax) - the kernel rounds P against THAT maximum and rescales only its
fp32 accumulator afterwards, so a restatement that rounded exp(S - max_j S) would draw another rounding pattern for every key in
front of the row's maximum, and against a reference that is itself rounded only the same pattern compares at the yardstick's scale.
It runs in the dtype of its operands (fp64: the reference of the GPU tests, fp32 on the GPU: the yardstick) and is differentiable:
every rounding is straight-through, d h(x) / dx = 1.  With ``rounding=False`` it is tests/token_attn_ref.py's operator
(tests/test_token_attn_half_host.py holds the two together at 1e-12)."""
from __future__ import annotations

import contextlib

import torch

from tests import token_attn_ref as R

U = 2.0 ** -11                      # unit roundoff of IEEE half
TILE = 64                           # keys per tile of the kernels' online softmax


def half(x, rounding=True):
    """x rounded to half and back, straight-through for gradients."""
    if not rounding:
        return x
    return x + (x.detach().to(torch.float16).to(x.dtype) - x.detach())


def token_attn(q, k, v, nh, scale, mask=None, rounding=True, factor=None):
    """q, k, v (B, C, T) -> (B, C, T); ``factor`` None or (B, nh, T, T): what each probability is multiplied by (dropout)."""
    b, c, t = q.shape
    hd = c // nh
    s = torch.einsum("bhci,bhcj->bhij", half(q * scale, rounding).reshape(b, nh, hd, t), half(k, rounding).reshape(b, nh, hd, t))
    if mask is not None:
        s = s.masked_fill(mask.reshape(b, 1, 1, t), float("-inf"))
    # the kernel's conversion point of P: key j of tile kt is exponentiated against the RUNNING maximum m_kt of its query row
    # (tiles 0 .. kt; a tile without a live key is skipped), rounded, and only the fp32 accumulator is rescaled afterwards by
    # w = exp(m_kt - m_last).  E W = exp(S - m_last) whatever the maxima are, so they carry no gradient.
    tiles = (t + TILE - 1) // TILE
    with torch.no_grad():
        pad = s.new_full((b, nh, t, tiles * TILE - t), float("-inf"))
        run = torch.cat((s, pad), dim=-1).reshape(b, nh, t, tiles, TILE).max(dim=-1).values.cummax(dim=-1).values
        last = run[..., -1:]
        run = torch.where(torch.isinf(run), last, run)              # in front of the first live tile: every key there is dead
        m = run.repeat_interleave(TILE, dim=-1)[..., :t]
        w = torch.exp(m - last)
    e = torch.exp(s - m)                                            # 0 at a dead key: the row keeps a live one, so m is finite
    den = (e * w).sum(dim=-1)
    if factor is not None:
        e = e * factor
    o = torch.einsum("bhij,bhcj->bhci", half(e, rounding) * w, half(v, rounding).reshape(b, nh, hd, t)) / den.unsqueeze(2)
    return o.reshape(b, c, t)


@contextlib.contextmanager
def rounded_attention(rounding=True):
    """While open, the module-level restatements of tests/token_attn_ref.py (``encoder_layer``, ``encoder``, and whatever calls
    them) compute their attention with the rounded operator above."""
    exact = R.token_attn
    R.token_attn = lambda q, k, v, n, scale, m=None: token_attn(q, k, v, n, scale, m, rounding)
    try:
        yield
    finally:
        R.token_attn = exact


def encoder(sd, src, num_layers, nh, activation, pre_norm, mask=None, pos=None, pe_only_at_begin=False, rounding=True):
    """tests/token_attn_ref.py's ``encoder`` with the attention above in the place of its exact one: (output, maps)."""
    with rounded_attention(rounding):
        return R.encoder(sd, src, num_layers, nh, activation, pre_norm, mask, pos, pe_only_at_begin)


def forward_bound(q, k, v, nh, scale, mask=None):
    """The a-priori bound on |o - o_exact| of one case, from its fp64 operands: operand rounding moves a score by at most
    delta = scale (2u + u^2) max_ij sum_c |q_ci| |k_cj| over live keys, so a softmax weight by a factor within exp(+-2 delta); 3u
    covers the rounding of P, of its sum and of v."""
    b, c, t = q.shape
    hd = c // nh
    a = torch.einsum("bhci,bhcj->bhij", q.abs().double().reshape(b, nh, hd, t), k.abs().double().reshape(b, nh, hd, t))
    if mask is not None:
        a = a.masked_fill(mask.reshape(b, 1, 1, t), 0.0)
    delta = scale * (2 * U + U * U) * float(a.max())
    return (float(torch.expm1(torch.tensor(2 * delta, dtype=torch.float64))) + 3 * U) * float(v.abs().max()) + 1e-6
