"""Temporal-encoder operators: LN + MLP, dense, the q/k/v front end, channel and local-window attention, the conv
embedding, linear upsampling and the flow-encoder blocks."""
from __future__ import annotations

import ctypes

import torch

from .. import hip
from .base import check_f32, require_gpu, _f32, _image, _launch


def ln_mlp_args(y, gamma, beta, eps, packed, scale, shift, out, hid):
    """Arguments of otp_ln_mlp_fused / otp_ln_mlp_x3 / otp_ln_mlp_h1 on a (B, C, T) tensor."""
    b, c, t = y.shape
    return (hip.ptr(y), hip.ptr(gamma), hip.ptr(beta), eps, hip.ptr(packed), hip.ptr(scale), hip.ptr(shift), hip.ptr(out), b, c, hid, t)


def ln_mlp_fused(y, gamma, beta, eps, packed, scale, shift, out=None, hid=None, stream=None, entry="otp_ln_mlp_fused"):
    """out = y + scale * (W2 . gelu(W1 . LN(y) + b1)) + shift: ln2 + MLP + residual of TransformerBlock.forward
    (model/blocks.py:277-279) in one launch."""
    require_gpu(y, packed)
    check_f32(y)
    hid = 4 * y.shape[1] if hid is None else hid
    out = torch.empty_like(y) if out is None else out
    _launch(getattr(hip.lib(), entry), entry, ln_mlp_args(y, gamma, beta, eps, packed, scale, shift, out, hid), y, stream)
    return out


def dense_cc_supported(c, t) -> bool:
    return bool(hip.lib().otp_dense_cc_supported(int(c), int(t)))


def dense_x3_supported(c, t) -> bool:
    return bool(hip.lib().otp_dense_x3_supported(int(c), int(t)))


def pack_dense_cc(weight, scale=None, shift=None, x3=False, grad=False):
    """(C, C[, 1]) pointwise weight (+ per-output-channel scale / shift) -> the per-16-row fragment image of
    :func:`dense_cc` (MaskedMHCA query / key / value / proj, model/blocks.py:383-386).  ``x3``: the split-half image of
    csrc/densex.hip (pass the same flag to :func:`dense_cc` / :func:`qkv_front`); ``grad`` (with ``x3``): the image with
    bfloat16 pieces for :func:`dense_cc` on operands of unknown magnitude - gradients (otp_bf16_pieces in csrc/densex.hip)."""
    require_gpu(weight)
    c = weight.shape[0]
    L = hip.lib()
    entry = ("otp_dense_x3_pack_bf16p" if grad else "otp_dense_x3_pack") if x3 else "otp_dense_cc_pack"
    nbytes = (L.otp_dense_x3_weight_bytes if x3 else L.otp_dense_cc_weight_bytes)(c) if weight.shape[1] == c else 0
    packed = _image(nbytes, torch.float32, weight.device, RuntimeError, f"otp_dense_cc: unsupported weight shape {tuple(weight.shape)}")
    w, sc, sh = (_f32(t, weight.device) for t in (weight, scale, shift))
    hip.check(getattr(L, entry)(hip.ptr(w), hip.ptr(sc), hip.ptr(sh), hip.ptr(packed), c, hip.stream_of(w)), entry)
    return packed


def dense_cc_args(xs, packs, ress, outs):
    """ctypes pointer arrays for :func:`dense_cc_launch` (kept by the caller while launches may still be issued)."""
    n = len(xs)
    arr = lambda ts: (ctypes.c_void_p * n)(*[hip.ptr(t) for t in ts])     # noqa: E731
    return arr(xs), arr(packs), arr(ress if ress is not None else [None] * n), arr(outs)


def dense_cc(xs, packs, ress=None, outs=None, stream=None, x3=False, grad=False, half=False):
    """out[p] = scale[p] * (W[p] . x[p]) + shift[p] (+ res[p]) for up to three (B, C, T) problems in one launch (``grad``: see
    :func:`pack_dense_cc`; ``half`` with ``x3``: the fp16 engine's arithmetic - operands rounded to half once, otp_dense_h1)."""
    require_gpu(*xs)
    b, c, t = xs[0].shape
    outs = [torch.empty_like(x) for x in xs] if outs is None else outs
    ax, ap, ar, ao = dense_cc_args(xs, packs, ress, outs)
    entry = ("otp_dense_x3_bf16p" if grad else "otp_dense_h1" if half else "otp_dense_x3") if x3 else "otp_dense_cc"
    hip.check(getattr(hip.lib(), entry)(ax, ap, ar, ao, len(xs), b, c, t, stream if stream is not None else hip.stream_of(xs[0])), entry)
    return outs


def pack_qkv_table(dwq, dwk, dwv, gq, bq, gk, bk, gv, bv):
    """Depthwise (C, 1, 3) weights and LayerNorm (C) gamma / beta of MaskedMHCA's query / key / value paths
    (model/blocks.py:359-381) -> the per-channel table of :func:`qkv_front`."""
    ts = [_f32(t) for t in (dwq, dwk, dwv, gq, bq, gk, bk, gv, bv)]
    require_gpu(*ts)
    c = ts[3].numel()
    L = hip.lib()
    table = torch.empty(L.otp_qkv_front_table_bytes(c) // 4, dtype=torch.float32, device=ts[0].device)
    hip.check(L.otp_qkv_front_pack_table(*[hip.ptr(t) for t in ts], hip.ptr(table), c, hip.stream_of(ts[0])),
              "otp_qkv_front_pack_table")
    return table


def qkv_front_args(x, table, packs, outs, eps):
    """Arguments of otp_qkv_front / otp_qkv_front_x3 / otp_qkv_front_h1."""
    b, c, t = x.shape
    return (hip.ptr(x), hip.ptr(table), *[hip.ptr(p) for p in packs], *[hip.ptr(o) for o in outs], b, c, t, eps)


def qkv_front(x, table, packs, eps=1e-5, outs=None, stream=None, x3=False, half=False):
    """q, k, v = W_p . LN_p(dwconv3_p(x)) + b_p (stride 1) in one launch; ``packs`` = three :func:`pack_dense_cc` images
    (``half`` with ``x3``: operands rounded to half once, otp_qkv_front_h1)."""
    require_gpu(x, table)
    outs = [torch.empty_like(x) for _ in range(3)] if outs is None else outs
    entry = ("otp_qkv_front_h1" if half else "otp_qkv_front_x3") if x3 else "otp_qkv_front"
    _launch(getattr(hip.lib(), entry), entry, qkv_front_args(x, table, packs, outs, eps), x, stream)
    return outs


def mlp_fused_supported(c, hid, t) -> bool:
    return bool(hip.lib().otp_mlp_fused_supported(int(c), int(hid), int(t)))


def pack_mlp_weights(w1, b1, w2):
    """Conv1d(C,4C,1) / Conv1d(4C,C,1) weights of a TransformerBlock MLP (model/blocks.py:248-254) -> the per-hidden-block
    fragment image :func:`mlp_fused` streams through LDS."""
    require_gpu(w1, b1, w2)
    hid, c = w1.shape[:2]
    L = hip.lib()
    packed = _image(L.otp_mlp_fused_weight_bytes(c, hid), torch.float32, w1.device,
                    RuntimeError, f"otp_mlp_fused: unsupported widths C={c}, HID={hid}")
    w1c, w2c, b1c = (_f32(t) for t in (w1, w2, b1))
    hip.check(L.otp_mlp_fused_pack(hip.ptr(w1c), hip.ptr(b1c), hip.ptr(w2c), hip.ptr(packed), c, hid, hip.stream_of(w1c)),
              "otp_mlp_fused_pack")
    return packed


def mlp_fused(x, packed, scale, shift, res, out=None, hid=None, stream=None, entry="otp_mlp_fused"):
    """out = res + scale * (W2 . gelu(W1 . x + b1)) + shift on (B, C, T) tensors, one launch (eval-mode MLP half of
    TransformerBlock.forward, model/blocks.py:277-279)."""
    require_gpu(x, packed, res)
    check_f32(x)
    b, c, t = x.shape
    hid = 4 * c if hid is None else hid
    out = torch.empty_like(x) if out is None else out
    _launch(getattr(hip.lib(), entry), entry, (hip.ptr(x), hip.ptr(packed), hip.ptr(scale), hip.ptr(shift), hip.ptr(res), hip.ptr(out),
                                                b, c, hid, t), x, stream)
    return out


def mlp_x3_supported(c, hid, t) -> bool:
    return bool(hip.lib().otp_mlp_x3_supported(int(c), int(hid), int(t)))


def pack_mlp_x3_weights(w1, b1, w2, half=False):
    """The same MLP weights as :func:`pack_mlp_weights`, split into half hi / lo MFMA fragments per 32 hidden channels
    (csrc/mlpx.hip); ``half``: the hi-only image of the fp16 engine's form (``ln_mlp_x3(..., half=True)``)."""
    require_gpu(w1, b1, w2)
    hid, c = w1.shape[:2]
    L = hip.lib()
    entry = "otp_mlp_h1" if half else "otp_mlp_x3"
    packed = _image(getattr(L, entry + "_weight_bytes")(c, hid), torch.int32, w1.device,
                    RuntimeError, f"otp_mlp_x3: unsupported widths C={c}, HID={hid}")
    w1c, w2c, b1c = (_f32(t) for t in (w1, w2, b1))
    hip.check(getattr(L, entry + "_pack")(hip.ptr(w1c), hip.ptr(b1c), hip.ptr(w2c), hip.ptr(packed), c, hid, hip.stream_of(w1c)),
              entry + "_pack")
    return packed


def mlp_x3(x, packed, scale, shift, res, out=None, hid=None, stream=None):
    """:func:`mlp_fused` with split-half products on the 16-bit matrix cores (fp32 storage / accumulation)."""
    return mlp_fused(x, packed, scale, shift, res, out, hid, stream, "otp_mlp_x3")


def ln_mlp_x3(y, gamma, beta, eps, packed, scale, shift, out=None, hid=None, stream=None, half=False):
    """:func:`ln_mlp_fused` with split-half products (``half``: operands and the hidden layer rounded to half once, otp_ln_mlp_h1)."""
    return ln_mlp_fused(y, gamma, beta, eps, packed, scale, shift, out, hid, stream, "otp_ln_mlp_h1" if half else "otp_ln_mlp_x3")


def ln_channel(x, gamma, beta, eps=1e-5, pool=False):
    require_gpu(x)
    b, c, t = x.shape
    y = torch.empty_like(x)
    p = torch.empty((b, c, (t + 2 - 3) // 2 + 1), dtype=x.dtype, device=x.device) if pool else None
    hip.check(hip.lib().otp_ln_channel(hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), hip.ptr(y), hip.ptr(p), b, c, t,
                                       eps, hip.stream_of(x)), "otp_ln_channel")
    return (y, p) if pool else y


def dwconv_ln3(x, dw, gammas, betas, stride, eps=1e-5):
    """dw / gammas / betas: triples for (query, key, value)."""
    require_gpu(x)
    b, c, t = x.shape
    to = (t + 2 - 3) // stride + 1
    outs = [torch.empty((b, c, to), dtype=x.dtype, device=x.device) for _ in range(3)]
    hip.check(hip.lib().otp_dwconv_ln3(
        hip.ptr(x), hip.ptr(dw[0]), hip.ptr(dw[1]), hip.ptr(dw[2]), hip.ptr(gammas[0]), hip.ptr(betas[0]),
        hip.ptr(gammas[1]), hip.ptr(betas[1]), hip.ptr(gammas[2]), hip.ptr(betas[2]), hip.ptr(outs[0]),
        hip.ptr(outs[1]), hip.ptr(outs[2]), b, c, t, stride, eps, hip.stream_of(x)), "otp_dwconv_ln3")
    return outs


def chan_attn_args(q, k, v, out, ws, nbytes, n_head, scale):
    b, c, t = q.shape
    return (hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(out), hip.ptr(ws), nbytes, b, c, t, n_head, scale)


def chan_attn(q, k, v, n_head, scale):
    require_gpu(q, k, v)
    b, c, t = q.shape
    out = torch.empty_like(q)
    L = hip.lib()
    nbytes = L.otp_chan_attn_workspace(b, c, t, n_head)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=q.device)
    _launch(L.otp_chan_attn, "otp_chan_attn", chan_attn_args(q, k, v, out, ws, nbytes, n_head, scale), q)
    return out


def check_local_attn(c, t, n_head, window_size):
    """Raise ``ValueError`` for a shape the local attention does not take (odd window 5 .. 33, ``t % (window_size - 1) == 0``:
    ``otp_local_attn_supported``)."""
    if n_head <= 0 or c % n_head:
        raise ValueError(f"local_attn: {c} channels do not split into {n_head} heads")
    if not hip.lib().otp_local_attn_supported(c // n_head, t, int(window_size)):
        raise ValueError(f"local_attn: window_size must be odd and in [5, 33] and the {t} tokens a multiple of window_size - 1, "
                         f"got window_size {window_size}")


def local_attn_args(q, k, v, rel_pe, out, probs, n_head, window_size, scale):
    b, c, t = q.shape
    return (hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(rel_pe), hip.ptr(out), hip.ptr(probs), b, c, t, n_head, int(window_size),
            scale)


def rel_pe_table(rel_pe, n_head, window_size, like):
    """``rel_pe`` ((1, 1, n_head, window_size) parameter or None) as the contiguous fp32 (n_head, window_size) table."""
    if rel_pe is None:
        return None
    if rel_pe.numel() != n_head * window_size:
        raise ValueError(f"local_attn: rel_pe has {rel_pe.numel()} entries, n_head * window_size is {n_head * window_size}")
    return rel_pe.detach().to(like.device, torch.float32).reshape(n_head, window_size).contiguous()


def local_attn(q, k, v, n_head, window_size, scale, rel_pe=None):
    """Local-window attention of LocalMaskedMHCA (model/blocks.py:479-833) on q, k, v (B, C, T): every token attends to the
    ``window_size`` positions centred on it, positions outside the sequence take no part; ``rel_pe`` (1, 1, n_head, window_size)
    is added to the scaled scores.  Returns (B, C, T) in the natural layout (csrc/localattn.hip, one launch)."""
    require_gpu(q, k, v)
    check_f32(q, k, v)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    b, c, t = q.shape
    check_local_attn(c, t, n_head, window_size)
    rel = rel_pe_table(rel_pe, n_head, window_size, q)
    out = torch.empty_like(q)
    _launch(hip.lib().otp_local_attn, "otp_local_attn", local_attn_args(q, k, v, rel, out, None, n_head, window_size, scale), q)
    return out


CONV_EMBD_KS = (1, 3, 5)              # the kernel sizes csrc/convembd.hip is built for
CONV_EMBD_MAX_CHANNELS = 256


def check_conv_embd(b, cin, h, w, cout, ks):
    """Raise ``ValueError`` for a shape the conv embedding does not take (``otp_conv_embd_supported``: ks 1 / 3 / 5, at most 256
    input and output channels)."""
    if (isinstance(ks, bool) or not isinstance(ks, int) or min(b, cin, h, w, cout) < 1
            or not hip.lib().otp_conv_embd_supported(b, cin, h, w, cout, ks)):
        raise ValueError(f"conv_embd: kernel size must be one of {CONV_EMBD_KS} and 1 <= channels <= {CONV_EMBD_MAX_CHANNELS}, got "
                         f"ks {ks}, {cin} -> {cout} channels on a ({b}, {cin}, {h}, {w}) input")


def pack_conv_embd_weight(weight):
    """(Cout, Cin, ks, ks) -> the packed [tap][Cin4][CoutP] device tensor of :func:`conv_embd` (csrc/convembd.hip)."""
    require_gpu(weight)
    check_f32(weight)
    w = _f32(weight)
    if w.dim() != 4 or w.shape[2] != w.shape[3]:
        raise ValueError(f"conv_embd: weight must be (Cout, Cin, ks, ks), got {tuple(weight.shape)}")
    cout, cin, ks, _ = w.shape
    L = hip.lib()
    nbytes = L.otp_conv_embd_weight_bytes(cin, cout, ks)
    if nbytes == 0:
        check_conv_embd(1, cin, 1, 1, cout, ks)
    wp = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    _launch(L.otp_conv_embd_pack_weight, "otp_conv_embd_pack_weight", (hip.ptr(w), hip.ptr(wp), cin, cout, ks), w)
    return wp


def conv_embd_params(x_shape, weight, bias, ln_weight, ln_bias, pe, device):
    """The checked, flattened fp32 forms (bias, gamma, beta, pe) of a conv embedding layer's optional arguments for an input of
    ``x_shape`` (B, Cin, H, W): ``ValueError`` for anything that does not fit."""
    if len(x_shape) != 4 or weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise ValueError(f"conv_embd: x must be (B, Cin, H, W) and weight (Cout, Cin, ks, ks), got {tuple(x_shape)} and "
                         f"{tuple(weight.shape)}")
    b, cin, h, w = x_shape
    cout, cin_w, ks, _ = weight.shape
    if cin_w != cin:
        raise ValueError(f"conv_embd: weight takes {cin_w} input channels, x has {cin}")
    check_conv_embd(b, cin, h, w, cout, int(ks))
    if (ln_weight is None) != (ln_bias is None):
        raise ValueError("conv_embd: ln_weight and ln_bias come together (both or neither)")
    flat = []
    for name, t in (("bias", bias), ("ln_weight", ln_weight), ("ln_bias", ln_bias)):
        if t is not None and t.numel() != cout:
            raise ValueError(f"conv_embd: {name} has {t.numel()} entries, the layer has {cout} output channels")
        flat.append(None if t is None else _f32(t, device).reshape(cout))
    if pe is not None:
        if pe.numel() != cout * h * w:
            raise ValueError(f"conv_embd: pe must hold ({cout}, {h * w}) entries, got {tuple(pe.shape)}")
        pe = _f32(pe, device).reshape(cout, h * w)
    return (*flat, pe)


def conv_embd_args(x, wpacked, bias, gamma, beta, pe, out, z, cout, ks, eps):
    b, cin, h, w = x.shape
    return (hip.ptr(x), hip.ptr(wpacked), hip.ptr(bias), hip.ptr(gamma), hip.ptr(beta), hip.ptr(pe), hip.ptr(out), hip.ptr(z),
            b, cin, h, w, cout, int(ks), float(eps))


def conv_embd(x, weight, bias, ln_weight, ln_bias, pe=None, eps=1e-5):
    """One conv embedding layer of ConvTransformer (ConvVideoTransformer.py:60-78, 129-135) as one launch in exact fp32:
    ``relu(LayerNorm_c(conv2d(x, weight, bias, padding=ks // 2))) (+ pe)`` on x (B, Cin, H, W) -> (B, Cout, H * W).  ``ln_weight`` /
    ``ln_bias`` ((1, Cout, 1) or None: no norm) are the channel LayerNorm of model/blocks.py:95-110, ``pe`` (Cout, H * W) is
    added behind the ReLU."""
    require_gpu(x, weight)
    check_f32(x, weight)
    x = x.contiguous()
    bias, gamma, beta, pe = conv_embd_params(x.shape, weight, bias, ln_weight, ln_bias, pe, x.device)
    cout, ks = weight.shape[0], weight.shape[2]
    out = torch.empty((x.shape[0], cout, x.shape[2] * x.shape[3]), dtype=torch.float32, device=x.device)
    _launch(hip.lib().otp_conv_embd, "otp_conv_embd",
            conv_embd_args(x, pack_conv_embd_weight(weight), bias, gamma, beta, pe, out, None, cout, ks, eps), x)
    return out


def upsample_linear_args(x, out, f, out_coff=0):
    """``x`` (B, C, T) or (B, C, H, W) with T = H * W, written to channels [out_coff, out_coff + C) of ``out``."""
    b, c = x.shape[:2]
    return (hip.ptr(x), hip.ptr(out), b, c, x.numel() // (b * c), f, out.shape[1], out_coff)


def upsample_linear(x, f, out=None, out_coff=0):
    require_gpu(x)
    b, c, t = x.shape
    if out is None:
        out = torch.empty((b, c, t * f), dtype=x.dtype, device=x.device)
    _launch(hip.lib().otp_upsample_linear, "otp_upsample_linear", upsample_linear_args(x, out, f, out_coff), x)
    return out


# ---- flow-encoder TransformerBlock (C = 17) as two launches around the channel attention (csrc/flowenc.hip) ---------------
def flow_block_supported(blk, c, t) -> bool:
    """Stride-1 TransformerBlock with 17 channels, biases everywhere and one epsilon for ln1 and the q / k / v norms."""
    a = blk.attn
    try:
        eps = {float(m.eps) for m in (blk.ln1, a.query_norm, a.key_norm, a.value_norm)}
        has_bias = all(m.bias is not None for m in (a.query, a.key, a.value, a.proj, blk.mlp[0], blk.mlp[3]))
        dw_ok = all(tuple(m.weight.shape) == (c, 1, 3) and m.bias is None for m in (a.query_conv, a.key_conv, a.value_conv))
    except AttributeError:
        return False
    return (len(eps) == 1 and has_bias and dw_ok
            and bool(hip.lib().otp_flow_block_supported(int(c), int(blk.mlp[0].out_channels), int(t))))


def pack_flow_front(blk, device):
    """Parameter block of ``otp_flow_front`` (layout: include/otpose_hip.h) from a TransformerBlock's modules."""
    a = blk.attn
    f = lambda t: t.detach().to(device, torch.float32).reshape(-1)                     # noqa: E731
    parts = [f(blk.ln1.weight), f(blk.ln1.bias)]
    for conv, norm, proj in ((a.query_conv, a.query_norm, a.query), (a.key_conv, a.key_norm, a.key),
                             (a.value_conv, a.value_norm, a.value)):
        parts += [f(conv.weight), f(norm.weight), f(norm.bias), f(proj.weight), f(proj.bias)]
    prm = torch.cat(parts).contiguous()
    c = blk.ln1.weight.numel()
    assert prm.numel() == hip.lib().otp_flow_front_param_floats(c), (prm.numel(), c)
    return prm


def pack_flow_back(blk, device):
    """Parameter block of ``otp_flow_back``: the drop-path scales (model/blocks.py:298-301, eval: plain per-channel factors)
    folded into the projection / down-projection rows and biases; W_2 transposed to (hidden, C)."""
    a = blk.attn
    d = lambda t: t.detach().to(device, torch.float32)                                 # noqa: E731
    c = blk.ln1.weight.numel()
    hid = blk.mlp[0].out_channels
    sa, sm = d(blk.drop_path_attn.scale).reshape(-1), d(blk.drop_path_mlp.scale).reshape(-1)
    wp = d(a.proj.weight).reshape(c, c) * sa[:, None]
    w2 = d(blk.mlp[3].weight).reshape(c, hid) * sm[:, None]
    parts = [wp.reshape(-1), d(a.proj.bias) * sa, d(blk.ln2.weight).reshape(-1), d(blk.ln2.bias).reshape(-1),
             d(blk.mlp[0].weight).reshape(-1), d(blk.mlp[0].bias), w2.t().contiguous().reshape(-1), d(blk.mlp[3].bias) * sm]
    prm = torch.cat(parts).contiguous()
    assert prm.numel() == hip.lib().otp_flow_back_param_floats(c, hid), (prm.numel(), c, hid)
    return prm


def flow_front_args(x, prm, q, k, v, eps):
    b, c, t = x.shape
    return (hip.ptr(x), hip.ptr(prm), hip.ptr(q), hip.ptr(k), hip.ptr(v), b, c, t, float(eps))


def flow_back_args(x, att, prm, out, hidden, eps):
    b, c, t = x.shape
    return (hip.ptr(x), hip.ptr(att), hip.ptr(prm), hip.ptr(out), b, c, int(hidden), t, float(eps))


def flow_front(x, prm, eps=1e-5):
    """q, k, v of a flow-encoder block from its input (B, 17, T)."""
    require_gpu(x, prm)
    check_f32(x)
    x = x.contiguous()
    q, k, v = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    _launch(hip.lib().otp_flow_front, "otp_flow_front", flow_front_args(x, prm, q, k, v, eps), x)
    return q, k, v


def flow_back(x, att, prm, hidden, eps=1e-5):
    """Block output from its input ``x`` and the attention output ``att`` (both (B, 17, T))."""
    require_gpu(x, att, prm)
    check_f32(x)
    x, att = x.contiguous(), att.contiguous()
    out = torch.empty_like(x)
    _launch(hip.lib().otp_flow_back, "otp_flow_back", flow_back_args(x, att, prm, out, hidden, eps), x)
    return out
