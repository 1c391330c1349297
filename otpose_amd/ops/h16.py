"""The fp16-storage eval kernels of the backbone (csrc/h16.hip; ``cfg.MODEL.DTYPE = "fp16"``)."""
from __future__ import annotations

import ctypes

import torch

from .. import hip
from .base import ACT_NONE, H8, View, require_gpu, _f32, _image, _launch, _slice, _vp
from .conv import stem_conv_x3_args


def h8_empty(n, c, h, w, device):
    nbytes = hip.lib().otp_h8_bytes(n, c, h, w)
    if not nbytes:
        raise ValueError(f"H8 images need a channel count that is a multiple of 8, got {c}")
    return H8(torch.empty(nbytes // 4, dtype=torch.int32, device=device), n, c, h, w)


def h8_pack(x, out: H8 = None, stream=None):
    """fp32 NCHW tensor or channel-slice :class:`View` -> H8 (one rounding to half per element)."""
    iv = x if isinstance(x, View) else View(x.contiguous())
    require_gpu(iv.t)
    n, _, h, w = iv.t.shape
    out = h8_empty(n, iv.C, h, w, iv.t.device) if out is None else out
    hip.check(hip.lib().otp_h8_pack(hip.ptr(iv.t), hip.ptr(out.t), n, iv.C, h, w, iv.ctot, iv.coff, out.gtot, out.goff,
                                    stream if stream is not None else hip.stream_of(iv.t)), "otp_h8_pack")
    return out


def h8_unpack(img: H8, stream=None):
    """H8 image -> fp32 (N, C, H, W), exact."""
    out = torch.empty(img.N, img.C, img.H, img.W, dtype=torch.float32, device=img.t.device)
    hip.check(hip.lib().otp_h8_unpack(hip.ptr(img.t), hip.ptr(out), img.N, img.C, img.H, img.W, img.gtot, img.goff,
                                      stream if stream is not None else hip.stream_of(img.t)), "otp_h8_unpack")
    return out


def h16_conv_desc(x: H8, cout, stride, act=ACT_NONE, out: H8 = None, res: H8 = None, k=0):
    d = hip.H16ConvDesc()
    d.N, d.Cin, d.H, d.W, d.Cout, d.stride, d.act = x.N, x.C, x.H, x.W, cout, stride, act
    d.in_gtot, d.in_goff = x.gtot, x.goff
    d.out_gtot, d.out_goff = (out.gtot, out.goff) if out is not None else (0, 0)
    d.res_gtot, d.res_goff = (res.gtot, res.goff) if res is not None else (0, 0)
    d.out_scale = 2.0 ** -k
    return d


def h16_conv_supported(desc) -> bool:
    return bool(hip.lib().otp_h16_conv3x3_supported(desc))


def pack_h16_conv_weight(weight, scale=None, k=0):
    """(Cout, Cin, 3, 3) fp32 (x scale[cout] x 2^k) -> the half A-fragment image of csrc/h16.hip."""
    require_gpu(weight)
    w = _f32(weight)
    cout, cin, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    L = hip.lib()
    packed = _image(L.otp_h16_conv3x3_weight_bytes(cout, cin), torch.int32, w.device,
                    RuntimeError, f"otp_h16_conv3x3: unsupported widths {cin} -> {cout}", zero=True)
    sc = _f32(scale, w.device)
    hip.check(L.otp_h16_conv3x3_pack_weight(hip.ptr(w), hip.ptr(sc), hip.ptr(packed), cout, cin, float(2.0 ** k), hip.stream_of(w)),
              "otp_h16_conv3x3_pack_weight")
    return packed


def h16_conv3x3_args(x: H8, wpacked, shift, out: H8, desc, res: H8 = None):
    return (_vp(x), hip.ptr(wpacked), hip.ptr(shift), _vp(res), _vp(out), desc)


def h16_conv3x3(x: H8, wpacked, shift, cout, stride=1, act=ACT_NONE, res: H8 = None, out: H8 = None, k=0, stream=None, desc=None):
    """out = act(conv3x3 pad 1 (x) + shift (+ res)) on H8 images (csrc/h16.hip)."""
    ho, wo = x.H // stride, x.W // stride
    out = h8_empty(x.N, cout, ho, wo, x.t.device) if out is None else out
    d = desc if desc is not None else h16_conv_desc(x, cout, stride, act, out, res, k)
    _launch(hip.lib().otp_h16_conv3x3, "otp_h16_conv3x3", h16_conv3x3_args(x, wpacked, shift, out, d, res), x.t, stream)
    return out


def h16_pointwise_supported(cin, cout) -> bool:
    return bool(hip.lib().otp_h16_pointwise_supported(int(cin), int(cout)))


def pack_h16_pointwise(weight, scale=None, shift=None, k=0):
    """(Cout, Cin[, 1, 1]) fp32 (x scale x 2^k) + shift -> the packed image of otp_h16_pointwise."""
    require_gpu(weight)
    w = _f32(weight.reshape(weight.shape[0], -1))
    cout, cin = w.shape
    L = hip.lib()
    packed = _image(L.otp_h16_pointwise_weight_bytes(cin, cout), torch.int32, w.device,
                    RuntimeError, f"otp_h16_pointwise: unsupported widths {cin} -> {cout}", zero=True)
    sc, sh = _f32(scale, w.device), _f32(shift, w.device)
    hip.check(L.otp_h16_pointwise_pack(hip.ptr(w), hip.ptr(sc), hip.ptr(sh), hip.ptr(packed), cin, cout, float(2.0 ** k),
                                       hip.stream_of(w)), "otp_h16_pointwise_pack")
    return packed


def h16_pointwise_args(x: H8, packed, cout, out, relu=False, res: H8 = None, k=0):
    """``out``: an :class:`H8`, or a :class:`View` of an fp32 NCHW tensor."""
    return (_vp(x), hip.ptr(packed), _vp(res), _vp(out), int(isinstance(out, View)), x.N, x.C, cout, x.H * x.W, x.gtot, x.goff,
            *_slice(res), *_slice(out), int(relu), float(2.0 ** -k))


def h16_pointwise(x: H8, packed, cout, relu=False, res: H8 = None, out=None, k=0, stream=None):
    """out = act(W x + shift (+ res)): ``out`` an :class:`H8` (default: fresh) or a :class:`View` of an fp32 NCHW tensor."""
    if out is None:
        out = h8_empty(x.N, cout, x.H, x.W, x.t.device)
    _launch(hip.lib().otp_h16_pointwise, "otp_h16_pointwise", h16_pointwise_args(x, packed, cout, out, relu, res, k), x.t, stream)
    return out


def pack_h16_stem(weight, scale=None, shift=None):
    require_gpu(weight)
    w = _f32(weight)
    cout = w.shape[0]
    L = hip.lib()
    packed = _image(L.otp_h16_stem_weight_bytes(cout), torch.int32, w.device,
                    RuntimeError, f"otp_h16_stem: unsupported width {cout}", zero=True)
    sc, sh = _f32(scale, w.device), _f32(shift, w.device)
    hip.check(L.otp_h16_stem_pack(hip.ptr(w), hip.ptr(sc), hip.ptr(sh), hip.ptr(packed), cout, hip.stream_of(w)), "otp_h16_stem_pack")
    return packed


def h16_stem(clip, packed, cout, frames, out: H8 = None, stream=None):
    """relu(conv3x3 s2 p1 of the frames of the fp32 clip (B, 3 F, H, W) + shift) as the H8 image of (F B, cout, Ho, Wo)."""
    require_gpu(clip)
    b, c, h, w = clip.shape
    assert c == 3 * frames and clip.is_contiguous()
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = h8_empty(frames * b, cout, ho, wo, clip.device) if out is None else out
    _launch(hip.lib().otp_h16_stem, "otp_h16_stem", stem_conv_x3_args(clip, packed, out, frames, cout), clip, stream)
    return out


def h16_upsample_add_args(lows, factors, res: H8, out: H8, relu=True):
    """(arguments, ctypes arrays the caller keeps alive while the launch may still be issued) on dense H8 images."""
    lp = (ctypes.c_void_p * len(lows))(*[_vp(v) for v in lows])
    fp = (ctypes.c_int * len(lows))(*[int(f) for f in factors])
    return (lp, fp, len(lows), _vp(res), _vp(out), res.N, res.C, res.H, res.W, int(relu)), (lp, fp)


def h16_upsample_add(lows, factors, res: H8, relu=True, out: H8 = None, stream=None):
    """out = act(res + sum_k nearest_up(lows[k], factors[k])) on dense H8 images."""
    assert res.gtot * 8 == res.C and all(l.gtot * 8 == l.C for l in lows)
    out = h8_empty(res.N, res.C, res.H, res.W, res.t.device) if out is None else out
    args, _keep = h16_upsample_add_args(lows, factors, res, out, relu)
    _launch(hip.lib().otp_h16_upsample_add, "otp_h16_upsample_add", args, res.t, stream)
    return out
