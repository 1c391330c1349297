"""Convolution wrappers and weight packers: fp32 direct, Winograd, small, split-product (x3), S8 and stride-2 S8, stem,
pointwise (plain, S8, pair) and the HRNet fuse rows' upsample-add."""
from __future__ import annotations

import ctypes
import math
import os

import torch

from .. import hip
from .base import ACT_NONE, H8, _K, View, check_f32, out_hw, require_gpu, _f32, _image, _launch, _slice, _vp


def pack_conv_weight(weight):
    """(Cout, Cin, kh, kw) -> packed [kh*kw][Cin][Cout16] device tensor for :func:`conv2d`."""
    require_gpu(weight)
    check_f32(weight)
    w = _f32(weight)
    if w.dim() == 3:                      # Conv1d weight (Cout, Cin, k) with k == 1
        w = w.unsqueeze(-1)
    cout, cin, kh, kw = w.shape
    cout16 = (cout + 15) // 16 * 16
    wp = torch.empty(kh * kw * cin * cout16, dtype=torch.float32, device=w.device)
    hip.check(hip.lib().otp_conv2d_pack_weight(hip.ptr(w), hip.ptr(wp), cout, cin, kh, kw, hip.stream_of(w)),
              "otp_conv2d_pack_weight")
    return wp


def conv_desc(inp: View, out: View, cout, kh, kw, stride, pad, dil, act=ACT_NONE, in2: View = None,
              res: View = None, res_up=1, frame_split=0, cin=None):
    d = hip.ConvDesc()
    n_in, _, h, w = inp.t.shape
    d.N = out.t.shape[0]
    d.Cin = inp.C if cin is None else cin
    d.H, d.W, d.Cout, d.kh, d.kw, d.stride, d.pad, d.dil = h, w, cout, kh, kw, stride, pad, dil
    d.in_ctot, d.in_coff = inp.ctot, inp.coff
    d.in2_ctot, d.in2_coff = (in2.ctot, in2.coff) if in2 is not None else (0, 0)
    d.out_ctot, d.out_coff = out.ctot, out.coff
    d.res_ctot, d.res_coff = (res.ctot, res.coff) if res is not None else (0, 0)
    d.res_up, d.act, d.frame_split = res_up, act, frame_split
    d.Ho, d.Wo = out_hw(h, w, kh, kw, stride, pad, dil)
    f = max(res_up, 1)
    assert out.t.shape[2] == d.Ho * f and out.t.shape[3] == d.Wo * f, (tuple(out.t.shape), d.Ho, d.Wo, f)
    assert out.C == cout
    if res is not None:
        assert res.t.shape[2:] == out.t.shape[2:] and res.C == cout
    if in2 is not None:
        assert in2.t.shape[2:] == inp.t.shape[2:] and in2.C == d.Cin
    if frame_split:
        assert d.N == n_in * (inp.ctot // d.Cin)
    else:
        assert d.N == n_in
    return d


def conv2d_args(inp: View, wpacked, scale, shift, out: View, desc, in2: View = None, res: View = None):
    return (_vp(inp), _vp(in2), hip.ptr(wpacked), hip.ptr(scale), hip.ptr(shift), _vp(res), _vp(out), desc)


def conv2d_launch(inp: View, wpacked, scale, shift, out: View, desc, in2: View = None, res: View = None, stream=None):
    _launch(hip.lib().otp_conv2d, "otp_conv2d", conv2d_args(inp, wpacked, scale, shift, out, desc, in2, res), out.t, stream)


def pack_wino_weight(weight):
    """(Cout, Cin, 3, 3) -> U[16][Cin][Cout16] = G g G^T device tensor for :func:`conv2d_wino_launch`."""
    require_gpu(weight)
    check_f32(weight)
    w = _f32(weight)
    cout, cin, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    L = hip.lib()
    u = torch.empty(L.otp_conv2d_wino_weight_bytes(cout, cin) // 4, dtype=torch.float32, device=w.device)
    hip.check(L.otp_conv2d_wino_pack_weight(hip.ptr(w), hip.ptr(u), cout, cin, hip.stream_of(w)), "otp_conv2d_wino_pack_weight")
    return u


def small_conv_supported(desc) -> bool:
    return bool(hip.lib().otp_conv3x3_small_supported(desc))


def pack_small_conv_weight(weight):
    """(Cout, Cin, 3, 3) -> the [ci][tap][co] image :func:`conv3x3_small` reads through the scalar cache."""
    require_gpu(weight)
    w = _f32(weight)
    cout, cin = w.shape[:2]
    L = hip.lib()
    wt = _image(L.otp_conv3x3_small_weight_bytes(cout, cin), torch.float32, w.device,
                ValueError, f"otp_conv3x3_small: unsupported channel counts ({cout}, {cin})")
    hip.check(L.otp_conv3x3_small_pack(hip.ptr(w), hip.ptr(wt), cout, cin, hip.stream_of(w)), "otp_conv3x3_small_pack")
    return wt


def conv3x3_small_args(inp: View, in2: View, wpacked, scale, shift, out: View, desc):
    return (_vp(inp), _vp(in2), hip.ptr(wpacked), hip.ptr(scale), hip.ptr(shift), _vp(out), desc)


def conv3x3_small(x, weight, scale=None, shift=None, act=ACT_NONE, in2=None):
    """act(scale * conv2d(x (+ in2), weight, 3x3, stride 1, pad 1) + shift) for <= 24 channels (csrc/conv_small.hip)."""
    require_gpu(x, weight)
    check_f32(x)
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    out = torch.empty(n, cout, h, w, dtype=torch.float32, device=x.device)
    iv, ov = View(x.contiguous()), View(out)
    i2 = View(in2.contiguous()) if in2 is not None else None
    d = conv_desc(iv, ov, cout, 3, 3, 1, 1, 1, act, i2)
    wt = pack_small_conv_weight(weight)
    _launch(hip.lib().otp_conv3x3_small, "otp_conv3x3_small", conv3x3_small_args(iv, i2, wt, scale, shift, ov, d), x)
    return out


def h16_weight_exponent(weight, scale=None) -> int:
    """Power of two k the fp16 engine stores a layer's (BatchNorm-folded) weights with: max |w * scale| * 2^k in [2^13, 2^14), so
    weights down to 2^-27 of the largest stay normal halves; the launch multiplies its fp32 sums by 2^-k (exact)."""
    w = weight.detach()
    m = w.abs().reshape(w.shape[0], -1).amax(dim=1)
    if scale is not None:
        m = m * scale.detach().abs().to(m.device, m.dtype)
    m = float(m.max())
    if not (m > 0.0 and math.isfinite(m)):
        return 0
    return max(-40, min(40, 14 - math.frexp(m)[1]))


def x3_weight_exponent(weight, scale=None) -> int:
    """The power of two k a layer's split-product weights are stored with: max |weight * scale| * 2^k lands in [2^13, 2^14).

    A weight is carried as two IEEE-half pieces hi + lo (csrc/common.h); `lo` is at most 2^-11 |w|, so for BatchNorm-folded
    weights of magnitude 1e-2 it is a SUBNORMAL half (spacing 2^-24) and the pair holds the weight to 2^-25 absolute - 17
    significand bits - and that error is the same for every pixel of every frame, so it does not average out over a layer's sum
    the way activation rounding does: it was the whole heat-map error of the split-product forward.  Scaled by
    2^k both pieces are normal (22 bits); the kernels multiply the accumulated sum by 2^-k (``otp_conv_desc.out_scale``; the
    pointwise kernels through their per-channel epilogue scale).  ``OTPOSE_X3_WSCALE=0`` stores the weights unscaled."""
    if os.environ.get("OTPOSE_X3_WSCALE", "1") == "0":
        return 0
    return h16_weight_exponent(weight, scale)


def _scaled_vec(scale, k, cout, device):
    """scale[cout] * 2^k as a contiguous fp32 vector (None when there is nothing to multiply by)"""
    sc = _f32(scale, device)
    if k == 0:
        return sc
    f = float(2.0 ** k)
    return sc * f if sc is not None else torch.full((cout,), f, dtype=torch.float32, device=device)


def pack_x3_weight(weight, scale=None, stride=1, k=0):
    """(Cout, Cin, k, k) fp32, k = 3 or 1 (times scale[cout] * 2^k) -> half hi / lo MFMA fragments for :func:`conv2d_x3_launch`
    (the chunking depends on the kernel size and the stride); the descriptor's ``out_scale`` must then be 2^-k
    (:func:`x3_weight_exponent`)."""
    require_gpu(weight)
    check_f32(weight)
    w = _f32(weight)
    if w.dim() == 3:
        w = w.unsqueeze(-1)
    cout, cin, kh, kw = w.shape
    assert kh == kw and kh in (1, 3)
    L = hip.lib()
    u = _image(L.otp_conv2d_x3_weight_bytes(cout, cin, kh, stride), torch.int32, w.device,
               ValueError, f"otp_conv2d_x3: unsupported channel counts ({cout}, {cin})")
    sc = _scaled_vec(scale, k, cout, w.device)
    hip.check(L.otp_conv2d_x3_pack_weight(hip.ptr(w), hip.ptr(sc), hip.ptr(u), cout, cin, kh, stride, hip.stream_of(w)),
              "otp_conv2d_x3_pack_weight")
    return u


def x3_supported(desc) -> bool:
    return bool(hip.lib().otp_conv2d_x3_supported(desc))


def conv2d_x3_args(inp: View, wpacked, shift, out: View, desc, res: View = None):
    return (_vp(inp), hip.ptr(wpacked), hip.ptr(shift), _vp(res), _vp(out), desc)


def conv2d_x3_launch(inp: View, wpacked, shift, out: View, desc, res: View = None, stream=None):
    _launch(hip.lib().otp_conv2d_x3, "otp_conv2d_x3", conv2d_x3_args(inp, wpacked, shift, out, desc, res), out.t, stream)


def conv2d_x3(x, weight, scale=None, shift=None, act=ACT_NONE, res=None, pad=1, dil=1, stride=1):
    """act(conv2d(x, weight, stride, pad, dil) * scale + shift + res) with split-half products (csrc/convx.hip)."""
    require_gpu(x, weight)
    n, cin, h, w = x.shape
    cout, k = weight.shape[0], weight.shape[2]
    ho, wo = out_hw(h, w, k, k, stride, pad, dil)
    out = torch.empty(n, cout, ho, wo, dtype=torch.float32, device=x.device)
    iv, ov = View(x.contiguous()), View(out)
    rv = View(res.contiguous()) if res is not None else None
    d = conv_desc(iv, ov, cout, k, k, stride, pad, dil, act, None, rv)
    e = x3_weight_exponent(weight, scale)
    d.out_scale = 2.0 ** -e
    conv2d_x3_launch(iv, pack_x3_weight(weight, scale, stride, e), shift, ov, d, rv)
    return out


# ---- split-record (S8) activations and the LDS-DMA fed 3x3 convolution (csrc/convs.hip) --------------------------------
S8_F32_C4, S8_F32_NCHW = _K["OTP_S8_F32_C4"], _K["OTP_S8_F32_NCHW"]


def s8_empty(n, c, h, w, device):
    """Storage of the S8 image of a logical (n, c, h, w) fp32 tensor: [n][c/8][2][h*w] records of 8 bf16 (hi | lo)."""
    nbytes = hip.lib().otp_s8_bytes(n, c, h, w)
    if not nbytes:
        raise ValueError(f"S8 images need a channel count that is a multiple of 8, got {c}")
    return torch.empty(nbytes // 4, dtype=torch.int32, device=device)


def c4_empty(n, c, h, w, device):
    """Storage of the C4 image [n][c/4][h*w][4] fp32 of a logical (n, c, h, w) tensor."""
    assert c % 4 == 0
    return torch.empty(n * c * h * w, dtype=torch.float32, device=device)


def s8_pack(inp, out=None, out_c4=None, stream=None):
    """fp32 NCHW tensor or channel-slice :class:`View` -> S8 image (hi = rne_bf16(x), lo = rne_bf16(x - hi)) and, when
    ``out_c4`` is given, the C4 image of the same values."""
    iv = inp if isinstance(inp, View) else View(inp.contiguous())
    require_gpu(iv.t)
    n, _, h, w = iv.t.shape
    out = s8_empty(n, iv.C, h, w, iv.t.device) if out is None else out
    hip.check(hip.lib().otp_s8_pack(hip.ptr(iv.t), hip.ptr(out), hip.ptr(out_c4), n, iv.C, h, w, iv.ctot, iv.coff,
                                    stream if stream is not None else hip.stream_of(iv.t)), "otp_s8_pack")
    return out


def s8_unpack(s8, n, c, h, w):
    """S8 image -> fp32 (n, c, h, w) = hi + lo (tests / debugging)."""
    require_gpu(s8)
    out = torch.empty(n, c, h, w, dtype=torch.float32, device=s8.device)
    hip.check(hip.lib().otp_s8_unpack(hip.ptr(s8), hip.ptr(out), n, c, h, w, hip.stream_of(s8)), "otp_s8_unpack")
    return out


def c4_unpack(c4, n, c, h, w):
    """C4 image -> fp32 NCHW (tests / debugging)."""
    require_gpu(c4)
    out = torch.empty(n, c, h, w, dtype=torch.float32, device=c4.device)
    hip.check(hip.lib().otp_c4_unpack(hip.ptr(c4), hip.ptr(out), n, c, h, w, hip.stream_of(c4)), "otp_c4_unpack")
    return out


def s8_conv_supported(desc) -> bool:
    return bool(hip.lib().otp_conv3x3_s8_supported(desc))


def s8_conv_desc(n, cin, cout, h, w, act=ACT_NONE, out: View = None, res: View = None, stride=1):
    """Descriptor of the S8 convolutions: 3x3, pad 1, (n, cin, h, w) -> (n, cout, h / stride, w / stride)."""
    d = hip.ConvDesc()
    d.N, d.Cin, d.H, d.W, d.Cout = n, cin, h, w, cout
    d.kh = d.kw = 3
    d.stride, d.pad, d.dil = stride, 1, 1
    d.in_ctot, d.in_coff, d.in2_ctot, d.in2_coff = cin, 0, 0, 0
    d.out_ctot, d.out_coff = (out.ctot, out.coff) if out is not None else (cout, 0)
    d.res_ctot, d.res_coff = (res.ctot, res.coff) if res is not None else (0, 0)
    d.res_up = 1
    d.act, d.Ho, d.Wo, d.frame_split = act, h // stride, w // stride, 0
    return d


def s8_s2_conv_desc(n, cin, cout, h, w, act=ACT_NONE, out: View = None, res: View = None):
    """Descriptor of the stride-2 S8 convolution (csrc/convs2.hip): (n, cin, h, w) -> (n, cout, h / 2, w / 2)."""
    return s8_conv_desc(n, cin, cout, h, w, act, out, res, stride=2)


def s8_s2_conv_supported(desc, nchw_out=True):
    return bool(hip.lib().otp_conv3x3_s2_s8_supported(desc, int(nchw_out)))


def conv3x3_s2_s8_args(in_s8, wpacked, shift, desc, res: View = None, out: View = None, out_s8=None):
    """``out``: the fp32 NCHW result (with the optional residual ``res``), or ``out_s8``: its S8 image (csrc/convs2.hip)."""
    return (hip.ptr(in_s8), hip.ptr(wpacked), hip.ptr(shift), _vp(res), _vp(out), hip.ptr(out_s8), desc)


def conv3x3_s2_s8(x_s8, shape, weight, scale=None, shift=None, act=ACT_NONE, res=None, out="nchw"):
    """act(conv2d(x, weight, 3x3, stride 2, pad 1) * scale + shift (+ res)) from the S8 image ``x_s8`` of logical ``shape``
    (n, cin, h, w).  ``out = "nchw"``: fp32 (n, cout, h / 2, w / 2) tensor (``res`` an fp32 tensor of that shape or None);
    ``out = "s8"``: the S8 image of the result (no residual)."""
    require_gpu(x_s8, weight)
    n, cin, h, w = shape
    cout = weight.shape[0]
    e = x3_weight_exponent(weight, scale)
    wp = pack_s8_weight(weight, scale, e)
    sh = shift.detach().contiguous().float() if shift is not None else None
    L = hip.lib()
    if out == "s8":
        assert res is None
        d = s8_s2_conv_desc(n, cin, cout, h, w, act)
        d.out_scale = 2.0 ** -e
        o8 = s8_empty(n, cout, h // 2, w // 2, x_s8.device)
        _launch(L.otp_conv3x3_s2_s8, "otp_conv3x3_s2_s8", conv3x3_s2_s8_args(x_s8, wp, sh, d, out_s8=o8), x_s8)
        return o8
    o = torch.empty(n, cout, h // 2, w // 2, dtype=torch.float32, device=x_s8.device)
    rv = View(res.contiguous()) if res is not None else None
    d = s8_s2_conv_desc(n, cin, cout, h, w, act, View(o), rv)
    d.out_scale = 2.0 ** -e
    _launch(L.otp_conv3x3_s2_s8, "otp_conv3x3_s2_s8", conv3x3_s2_s8_args(x_s8, wp, sh, d, rv, View(o)), x_s8)
    return o


def pack_s8_weight(weight, scale=None, k=0):
    """(Cout, Cin, 3, 3) fp32 (times scale[cout] * 2^k) -> half hi / lo MFMA fragments for :func:`conv3x3_s8_launch` and
    :func:`conv3x3_s2_s8`; the descriptor's ``out_scale`` must then be 2^-k (:func:`x3_weight_exponent`)."""
    require_gpu(weight)
    check_f32(weight)
    w = _f32(weight)
    cout, cin, kh, kw = w.shape
    assert kh == kw == 3
    L = hip.lib()
    u = _image(L.otp_conv3x3_s8_weight_bytes(cout, cin), torch.int32, w.device,
               ValueError, f"otp_conv3x3_s8: unsupported channel counts ({cout}, {cin})")
    sc = _scaled_vec(scale, k, cout, w.device)
    hip.check(L.otp_conv3x3_s8_pack_weight(hip.ptr(w), hip.ptr(sc), hip.ptr(u), cout, cin, hip.stream_of(w)),
              "otp_conv3x3_s8_pack_weight")
    return u


def conv3x3_s8_args(in_s8, wpacked, shift, desc, res=None, out_f32=None, f32_layout=S8_F32_C4, out_s8=None):
    """``res``: the residual's C4 image, or its S8 image with ``desc.res_layout = 1``; ``out_f32``: a C4 image or an NCHW tensor."""
    return (hip.ptr(in_s8), hip.ptr(wpacked), hip.ptr(shift), hip.ptr(res), hip.ptr(out_f32), f32_layout, hip.ptr(out_s8), desc)


def conv3x3_s8_launch(in_s8, wpacked, shift, desc, res_c4=None, out_f32=None, f32_layout=S8_F32_C4, out_s8=None, stream=None):
    _launch(hip.lib().otp_conv3x3_s8, "otp_conv3x3_s8",
            conv3x3_s8_args(in_s8, wpacked, shift, desc, res_c4, out_f32, f32_layout, out_s8), in_s8, stream)


def conv3x3_s8(x_s8, shape, weight, scale=None, shift=None, act=ACT_NONE, res_c4=None, f32="nchw", want_s8=True, res_s8=None):
    """act(conv2d(x, weight, 3x3, stride 1, pad 1) * scale + shift + res) from an S8 image ``x_s8`` of logical ``shape``
    (n, cin, h, w); ``res_c4`` a C4 image of the residual.  Returns (fp32 result - an NCHW tensor for f32 = "nchw", a C4 image
    for "c4", None for None -, S8 image of the result or None)."""
    require_gpu(x_s8, weight)
    n, cin, h, w = shape
    cout = weight.shape[0]
    out = out_s8 = None
    layout = S8_F32_C4
    if f32 == "nchw":
        out, layout = torch.empty(n, cout, h, w, dtype=torch.float32, device=x_s8.device), S8_F32_NCHW
    elif f32 == "c4":
        out = c4_empty(n, cout, h, w, x_s8.device)
    if want_s8:
        out_s8 = s8_empty(n, cout, h, w, x_s8.device)
    d = s8_conv_desc(n, cin, cout, h, w, act)
    e = x3_weight_exponent(weight, scale)
    d.out_scale = 2.0 ** -e
    if res_s8 is not None:                           # the residual as S8 records (its hi + lo) instead of a C4 fp32 image
        assert res_c4 is None
        d.res_layout = 1
    conv3x3_s8_launch(x_s8, pack_s8_weight(weight, scale, e), shift, d, res_s8 if res_s8 is not None else res_c4, out, layout,
                      out_s8)
    return out, out_s8


def stem_conv_x3_supported(b, f, h, w, cout) -> bool:
    return bool(hip.lib().otp_stem_conv_x3_supported(int(b), int(f), int(h), int(w), int(cout)))


def pack_stem_conv_x3(weight, scale=None, shift=None):
    """(Cout, 3, 3, 3) weight of HRNet's first conv (+ folded BatchNorm) -> the register image of :func:`stem_conv_x3`."""
    require_gpu(weight)
    cout = weight.shape[0]
    L = hip.lib()
    nbytes = L.otp_stem_conv_x3_weight_bytes(cout) if tuple(weight.shape[1:]) == (3, 3, 3) else 0
    packed = _image(nbytes, torch.float32, weight.device, RuntimeError, f"otp_stem_conv_x3: unsupported weight shape {tuple(weight.shape)}")
    w, sc, sh = (_f32(t, weight.device) for t in (weight, scale, shift))
    hip.check(L.otp_stem_conv_x3_pack(hip.ptr(w), hip.ptr(sc), hip.ptr(sh), hip.ptr(packed), cout, hip.stream_of(w)),
              "otp_stem_conv_x3_pack")
    return packed


def stem_conv_x3_args(clip, packed, out, frames, cout):
    """Arguments of otp_stem_conv_x3 / otp_h16_stem: ``clip`` (B, 3 * frames, H, W) fp32, ``out`` a tensor or an :class:`H8`."""
    b, _, h, w = clip.shape
    return (hip.ptr(clip), hip.ptr(packed), hip.ptr(out.t if isinstance(out, H8) else out), b, frames, h, w, cout)


def stem_conv_x3(clip, packed, cout, frames=5, out=None, stream=None):
    """relu(bn(conv3x3 stride 2 pad 1)) of the 3-channel frames of ``clip`` (B, 3 * frames, H, W) -> (frames * B, cout, Ho, Wo),
    frame-major like model/OTPose.py:317."""
    require_gpu(clip)
    b, c, h, w = clip.shape
    assert c == 3 * frames and clip.is_contiguous() and clip.dtype == torch.float32
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = torch.empty(frames * b, cout, ho, wo, dtype=torch.float32, device=clip.device) if out is None else out
    _launch(hip.lib().otp_stem_conv_x3, "otp_stem_conv_x3", stem_conv_x3_args(clip, packed, out, frames, cout), clip, stream)
    return out


def pointwise_x3_supported(cin, cout, t) -> bool:
    return bool(hip.lib().otp_pointwise_x3_supported(int(cin), int(cout), int(t)))


def _pointwise_operands(weight, scale, shift, cout, cin, device):
    """fp32 (cout, cin) weight, scale, shift of a pointwise packer on ``device``: the weights stored times 2^e
    (:func:`x3_weight_exponent`), undone by the kernel's per-channel epilogue scale."""
    w, sc, sh = _f32(weight, device).reshape(cout, cin), _f32(scale, device), _f32(shift, device)
    e = x3_weight_exponent(w)
    if e:
        w, sc = w * float(2.0 ** e), _scaled_vec(sc, -e, cout, w.device)
    return w, sc, sh


def _pack_pointwise(entry, weight, scale, shift):
    """(Cout, Cin[, 1, 1]) weight (+ per-output-channel scale / shift) -> the image ``<entry>_pack`` writes."""
    require_gpu(weight)
    cout, cin = weight.shape[:2]
    L = hip.lib()
    packed = _image(getattr(L, entry + "_weight_bytes")(cin, cout), torch.float32, weight.device,
                    RuntimeError, f"{entry}: unsupported weight shape {tuple(weight.shape)}")
    w, sc, sh = _pointwise_operands(weight, scale, shift, cout, cin, weight.device)
    hip.check(getattr(L, entry + "_pack")(hip.ptr(w), hip.ptr(sc), hip.ptr(sh), hip.ptr(packed), cin, cout, hip.stream_of(w)),
              entry + "_pack")
    return packed


def pack_pointwise_x3(weight, scale=None, shift=None):
    """(Cout, Cin[, 1, 1]) weight (+ per-output-channel scale / shift, e.g. a folded BatchNorm) -> the block image of
    :func:`pointwise_x3` (HRNet layer1's 1x1 convs, model/HRNet.py:551-571)."""
    return _pack_pointwise("otp_pointwise_x3", weight, scale, shift)


def pointwise_x3_args(x: View, packed, out: View, res: View = None, relu=False):
    b, _, h, w = x.t.shape
    return (_vp(x), hip.ptr(packed), _vp(res), _vp(out), b, x.C, out.C, h * w, x.ctot, x.coff, *_slice(res), out.ctot, out.coff,
            int(bool(relu)))


def pointwise_x3(x: View, packed, out: View, res: View = None, relu=False, stream=None):
    """out = act(scale * (W . x) + shift (+ res)) over channel-slice views of (B, ctot, H, W) fp32 tensors."""
    require_gpu(x.t, out.t)
    _launch(hip.lib().otp_pointwise_x3, "otp_pointwise_x3", pointwise_x3_args(x, packed, out, res, relu), x.t, stream)
    return out


def pointwise_x3_s8_supported(cin, cout, t) -> bool:
    return bool(hip.lib().otp_pointwise_x3_s8_supported(int(cin), int(cout), int(t)))


def pack_pointwise_x3_s8(weight, scale=None, shift=None):
    """Weight image of :func:`pointwise_x3_s8` (its own row order: pairs of 16-row tiles interleaved by groups of 4)."""
    return _pack_pointwise("otp_pointwise_x3_s8", weight, scale, shift)


def pointwise_x3_s8_res_args(x: View, packed, cout, out_s8, res: View = None, relu=False):
    b, _, h, w = x.t.shape
    return (_vp(x), hip.ptr(packed), _vp(res), hip.ptr(out_s8), b, x.C, cout, h * w, x.ctot, x.coff, *_slice(res), int(bool(relu)))


def pointwise_x3_s8(x: View, packed, cout, out_s8=None, relu=False, stream=None, res: View = None):
    """S8 image of act(scale * (W . x) + shift (+ res)): a 1x1 conv feeding :func:`conv3x3_s8_launch` without an fp32 round trip
    (``res``: an fp32 NCHW channel-slice view, a Bottleneck's conv3)."""
    require_gpu(x.t)
    b, _, h, w = x.t.shape
    out_s8 = s8_empty(b, cout, h, w, x.t.device) if out_s8 is None else out_s8
    _launch(hip.lib().otp_pointwise_x3_s8_res, "otp_pointwise_x3_s8_res", pointwise_x3_s8_res_args(x, packed, cout, out_s8, res, relu),
            x.t, stream)
    return out_s8


def pointwise_x3_pair_supported(cin, cmid, cout2, t) -> bool:
    return bool(hip.lib().otp_pointwise_x3_pair_supported(int(cin), int(cmid), int(cout2), int(t)))


def pack_pointwise_x3_pair(weight1, scale1, shift1, weight2, scale2=None, shift2=None):
    """Weight image of :func:`pointwise_x3_pair`: conv3 (Cmid, Cin) of one Bottleneck and conv1 (Cout2, Cmid) of the next, each
    with its folded BatchNorm - the two images of :func:`pack_pointwise_x3_s8` in one buffer."""
    require_gpu(weight1, weight2)
    cmid, cin = weight1.shape[:2]
    cout2 = weight2.shape[0]
    L = hip.lib()
    nbytes = L.otp_pointwise_x3_pair_weight_bytes(cin, cmid, cout2) if weight2.shape[1] == cmid else 0
    packed = _image(nbytes, torch.float32, weight1.device, RuntimeError,
                    f"otp_pointwise_x3_pair: unsupported weight shapes {tuple(weight1.shape)}, {tuple(weight2.shape)}")
    ws = [*_pointwise_operands(weight1, scale1, shift1, cmid, cin, weight1.device),
          *_pointwise_operands(weight2, scale2, shift2, cout2, cmid, weight1.device)]
    hip.check(L.otp_pointwise_x3_pair_pack(*[hip.ptr(t) for t in ws], hip.ptr(packed), cin, cmid, cout2, hip.stream_of(ws[0])),
              "otp_pointwise_x3_pair_pack")
    return packed


def pointwise_x3_pair_args(x: View, packed, out: View, cout2, out_s8, res: View = None, relu1=True, relu2=True):
    b, _, h, w = x.t.shape
    return (_vp(x), hip.ptr(packed), _vp(res), _vp(out), hip.ptr(out_s8), b, x.C, out.C, cout2, h * w, x.ctot, x.coff, *_slice(res),
            out.ctot, out.coff, int(bool(relu1)), int(bool(relu2)))


def pointwise_x3_pair(x: View, packed, out: View, cout2, res: View = None, out_s8=None, relu1=True, relu2=True, stream=None):
    """out = act1(scale1 * (W1 . x) + shift1 (+ res)) as :func:`pointwise_x3` writes it AND the S8 image of
    act2(scale2 * (W2 . out) + shift2) as :func:`pointwise_x3_s8` of ``out`` writes it, in one launch; returns the S8 image."""
    require_gpu(x.t, out.t)
    b, _, h, w = x.t.shape
    out_s8 = s8_empty(b, cout2, h, w, x.t.device) if out_s8 is None else out_s8
    _launch(hip.lib().otp_pointwise_x3_pair, "otp_pointwise_x3_pair",
            pointwise_x3_pair_args(x, packed, out, cout2, out_s8, res, relu1, relu2), x.t, stream)
    return out_s8


def wino_supported(desc) -> bool:
    return bool(hip.lib().otp_conv2d_wino_supported(desc))


def winograd_pays(cin, cout):
    """Shapes on which the Winograd kernel measured faster than the direct one (tools/conv_bench.py --wino): whole
    8-channel chunks and output-channel counts that fill its 48-row tiles (64 -> 64 would compute 96 rows)."""
    cout16 = (cout + 15) // 16 * 16
    if cin == 64 and cout16 == 64:
        return True                                   # layer1 Bottleneck conv2: 0.463 -> 0.408 ms despite the ragged 2nd tile
    return cin >= 32 and cin % 8 == 0 and cout16 >= 48 and ((cout16 + 47) // 48) * 48 <= 1.15 * cout16


def runs_winograd(enabled, cin, cout, desc) -> bool:
    """The one rule for "this convolution runs on the Winograd kernel" (inference engine and training operators alike): the
    OTPOSE_WINOGRAD switch is on (``enabled``), 3x3 / stride 1 / pad 1 / dilation 1, the shape pays and the kernel takes it."""
    return bool(enabled and (desc.kh, desc.kw, desc.stride, desc.pad, desc.dil) == (3, 3, 1, 1, 1)
                and winograd_pays(cin, cout) and wino_supported(desc))


def conv2d_wino_args(inp: View, upacked, scale, shift, out: View, desc, res: View = None):
    return (_vp(inp), hip.ptr(upacked), hip.ptr(scale), hip.ptr(shift), _vp(res), _vp(out), desc)


def conv2d_wino_launch(inp: View, upacked, scale, shift, out: View, desc, res: View = None, stream=None):
    _launch(hip.lib().otp_conv2d_wino, "otp_conv2d_wino", conv2d_wino_args(inp, upacked, scale, shift, out, desc, res), out.t, stream)


def conv2d_wino(x, weight, scale=None, shift=None, act=ACT_NONE, res=None):
    """3x3 / stride 1 / pad 1 convolution through the Winograd F(2x2, 3x3) kernel, fresh output."""
    require_gpu(x, weight)
    cout = weight.shape[0]
    out = torch.empty((x.shape[0], cout, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
    iv, ov = View(x.contiguous()), View(out)
    rv = View(res.contiguous()) if res is not None else None
    d = conv_desc(iv, ov, cout, 3, 3, 1, 1, 1, act, None, rv, 1)
    conv2d_wino_launch(iv, pack_wino_weight(weight), scale, shift, ov, d, rv)
    return out


def conv2d(x, weight, scale=None, shift=None, stride=1, pad=0, dil=1, act=ACT_NONE, res=None, in2=None, res_up=1):
    """Convenience form: out = act(scale * conv(x (+ in2), weight) + shift (+ res)), fresh output."""
    require_gpu(x, weight)
    w4 = weight if weight.dim() == 4 else weight.unsqueeze(-1)
    cout, cin, kh, kw = w4.shape
    h, w = x.shape[2:]
    ho, wo = out_hw(h, w, kh, kw, stride, pad, dil)
    out = torch.empty((x.shape[0], cout, ho * max(res_up, 1), wo * max(res_up, 1)), dtype=torch.float32, device=x.device)
    iv, ov = View(x.contiguous()), View(out)
    rv = View(res.contiguous()) if res is not None else None
    i2 = View(in2.contiguous()) if in2 is not None else None
    d = conv_desc(iv, ov, cout, kh, kw, stride, pad, dil, act, i2, rv, res_up)
    conv2d_launch(iv, pack_conv_weight(w4), scale, shift, ov, d, i2, rv)
    return out


def upsample_add_args(low: View, res: View, out: View, f, relu=False):
    n, _, hl, wl = low.t.shape
    return (_vp(low), _vp(res), _vp(out), n, low.C, hl, wl, f, int(relu), low.ctot, low.coff, res.ctot, res.coff, out.ctot, out.coff)


def upsample_add(low, res, f, relu=False, out=None):
    """out = act(res + nearest_upsample_f(low)) (HRNet fuse accumulate for f >= 4); ``out`` may be ``res``."""
    require_gpu(low, res)
    out = torch.empty_like(res) if out is None else out
    _launch(hip.lib().otp_upsample_add, "otp_upsample_add", upsample_add_args(View(low), View(res), View(out), f, relu), low)
    return out


def upsample_add_multi_args(lows, factors, res: View, out: View, relu=False):
    """(arguments, ctypes arrays the caller keeps alive while the launch may still be issued); ``lows``: whole-tensor Views."""
    n, _, hh, wh = out.t.shape
    lp = (ctypes.c_void_p * len(lows))(*[_vp(v) for v in lows])
    fp = (ctypes.c_int * len(lows))(*[int(f) for f in factors])
    return (lp, fp, len(lows), _vp(res), _vp(out), n, res.C, hh, wh, int(relu), res.ctot, res.coff, out.ctot, out.coff), (lp, fp)


def upsample_add_multi(lows, res, relu=False, out=None):
    """out = act(res + sum_k nearest_upsample(lows[k])) in one pass (an HRNet fuse row's upsampled terms, summed in list
    order); each ``lows[k]`` is (N, C, H / f_k, W / f_k) with f_k a power of two >= 2."""
    require_gpu(res, *lows)
    n, c, hh, wh = res.shape
    out = torch.empty_like(res) if out is None else out
    lows = [t.contiguous() for t in lows]
    args, _keep = upsample_add_multi_args([View(t) for t in lows], [hh // t.shape[2] for t in lows], View(res), View(out), relu)
    _launch(hip.lib().otp_upsample_add_multi, "otp_upsample_add_multi", args, res)
    return out
