"""Plain torch restatements of the forward operators of the temporal and flow encoders (no GPU import), written so that they
work in whatever float dtype their operands have: in float64 they are the reference of tests/test_gpu_encoder_fwd.py, in
float32 on the CPU the yardstick its bounds are taken from (the pattern of tests/encoder_bwd_ref.py, whose channel LayerNorm
and channel attention expressions are reused here).  Written from the reference model's definitions: channel LayerNorm
(model/blocks.py:95-110), the depthwise q / k / v convs and their norms (:359-381, 406-416), the pointwise projections
(:383-386, 417-419, 450), the MLP (:248-254) and the residual / drop-path lines of TransformerBlock.forward (:264-280, eval
mode: the drop-path is its per-channel scale).  tests/test_encoder_fwd_host.py pins them against oracle/otpose_oracle.py run on
the state dict of a seeded modules.TransformerBlock."""
import torch
import torch.nn.functional as F

from tests.encoder_bwd_ref import chan_attn_expr, dwconv3_out_len, layer_norm_expr  # noqa: F401  (re-exported)


def _col(v):
    return None if v is None else v.reshape(1, -1, 1)


def layer_norm(x, gamma, beta, eps=1e-5):
    """Channel LayerNorm of (B, C, T): biased variance of the centred values, eps inside the root."""
    return layer_norm_expr(x, gamma, beta, eps)


def dwconv3(x, w, stride=1):
    """Depthwise Conv1d(C, C, 3, stride, padding 1, no bias) of (B, C, T) with w (C, 1, 3), tap by tap on the zero-padded row."""
    c = x.shape[1]
    to = dwconv3_out_len(x.shape[2], stride)
    xp = F.pad(x, (1, 1))
    w = w.reshape(c, 3)
    return sum(w[:, k].reshape(1, c, 1) * xp[:, :, k: k + stride * (to - 1) + 1: stride] for k in range(3))


def dwconv_ln3(x, dws, gammas, betas, stride, eps=1e-5):
    """The three depthwise convs of one input, each followed by its channel LayerNorm (otp_dwconv_ln3)."""
    return [layer_norm(dwconv3(x, dws[i], stride), gammas[i], betas[i], eps) for i in range(3)]


def pointwise(x, w, bias=None, scale=None, res=None):
    """Conv1d(C, C, 1) with the residual line of TransformerBlock.forward: [res +] [scale *] (W . x + bias); w (C, C[, 1])."""
    y = torch.einsum("oc,bct->bot", w.reshape(w.shape[0], -1), x)
    if bias is not None:
        y = y + _col(bias)
    if scale is not None:
        y = y * _col(scale)
    return y if res is None else res + y


def qkv_front(x, dws, gammas, betas, ws, bs, eps=1e-5):
    """q, k, v = W_p . LN_p(dwconv3_p(x)) + b_p at stride 1 (otp_qkv_front*)."""
    return [pointwise(n, ws[i], bs[i]) for i, n in enumerate(dwconv_ln3(x, dws, gammas, betas, 1, eps))]


def mlp(x, w1, b1, w2, b2, scale, res):
    """res + scale * (W2 . gelu(W1 . x + b1) + b2): the kernels take ``shift = b2 * scale`` (ops.mlp_fused)."""
    return pointwise(F.gelu(pointwise(x, w1, b1)), w2, b2, scale, res)


def ln_mlp(y, gamma, beta, eps, w1, b1, w2, b2, scale):
    """y + scale * (W2 . gelu(W1 . LN(y) + b1) + b2): ln2 + MLP + residual with the drop-path scale folded as ops.ln_mlp_fused
    documents it (``shift = b2 * scale``)."""
    return mlp(layer_norm(y, gamma, beta, eps), w1, b1, w2, b2, scale, y)


# ---- flow encoder (C = 17) from the parameter blocks of ops.pack_flow_front / pack_flow_back ---------------------------------------
def split_flow_front(prm, c):
    """front block: ln1 gamma[C], beta[C]; then for q, k, v: dw[C][3], norm gamma[C], norm beta[C], W[C][C] (out, in), bias[C]."""
    assert prm.numel() == 2 * c + 3 * (3 * c + 2 * c + c * c + c)
    parts, o = {"ln1": (prm[:c], prm[c: 2 * c])}, 2 * c
    for name in "qkv":
        dw, o = prm[o: o + 3 * c].reshape(c, 1, 3), o + 3 * c
        g, o = prm[o: o + c], o + c
        b, o = prm[o: o + c], o + c
        w, o = prm[o: o + c * c].reshape(c, c), o + c * c
        bias, o = prm[o: o + c], o + c
        parts[name] = (dw, g, b, w, bias)
    return parts


def flow_front(x, prm, eps=1e-5):
    """q, k, v = Conv1d_1x1(LN(dwconv3(ln1(x)))): the depthwise conv pads the ln1 OUTPUT with zeros."""
    p = split_flow_front(prm, x.shape[1])
    n = layer_norm(x, *p["ln1"], eps)
    br = [p[k] for k in "qkv"]
    return qkv_front(n, [b[0] for b in br], [b[1] for b in br], [b[2] for b in br], [b[3] for b in br], [b[4] for b in br], eps)


def split_flow_back(prm, c, hidden):
    """back block: W_p[C][C] * s_a[out], b_p * s_a; ln2 gamma, beta; W_1[H][C], b_1[H]; W_2^T[H][C] * s_m[out], b_2 * s_m."""
    assert prm.numel() == c * c + c + 2 * c + hidden * c + hidden + hidden * c + c
    sizes = [c * c, c, c, c, hidden * c, hidden, hidden * c, c]
    wp, bp, g, b, w1, b1, w2t, b2 = torch.split(prm, sizes)
    return wp.reshape(c, c), bp, g, b, w1.reshape(hidden, c), b1, w2t.reshape(hidden, c), b2


def flow_back(x, att, prm, hidden, eps=1e-5):
    """y = x + (W_p' att + b_p'); out = y + (W_2' gelu(W_1 ln2(y) + b_1) + b_2'), the primes carrying the folded drop-path scales."""
    wp, bp, g, b, w1, b1, w2t, b2 = split_flow_back(prm, x.shape[1], hidden)
    y = pointwise(att, wp, bp, None, x)
    return mlp(layer_norm(y, g, b, eps), w1, b1, w2t.t(), b2, None, y)
