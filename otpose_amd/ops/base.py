"""What every operator module shares: the header's constants, the device / dtype / shape checks, the tensor-slice
types (:class:`View`, :class:`H8`) and the launch helpers.  Imports ``hip`` alone."""
from __future__ import annotations

import torch

from .. import hip

_K = hip.CONSTANTS              # the OTP_* integers of include/otpose_hip.h


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NotImplementedError("otpose_amd operators run on the GPU only (no CPU path)")


def check_f32(*tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"otpose_amd HIP operators are built for float32, got {t.dtype}")


def out_hw(h, w, kh, kw, stride, pad, dil):
    """Output size of a convolution (the one statement of it: train_ops and bf16_ops call this too)."""
    return ((h + 2 * pad - (dil * (kh - 1) + 1)) // stride + 1,
            (w + 2 * pad - (dil * (kw - 1) + 1)) // stride + 1)


def _f32(t, device=None):
    """Detached contiguous fp32 form of an optional tensor, on ``device`` (default: where it is); ``None`` stays ``None``."""
    return None if t is None else t.detach().to(t.device if device is None else device, torch.float32).contiguous()


def _image(nbytes, dtype, device, exc, what, zero=False):
    """Storage of a packed image: ``nbytes`` is what the entry point's ``*_weight_bytes`` answered, 0 meaning that it has
    no kernel for the shape (``exc(what)``); 4-byte elements of ``dtype``, zero-filled on request."""
    if not nbytes:
        raise exc(what)
    return (torch.zeros if zero else torch.empty)(nbytes // 4, dtype=dtype, device=device)


def _tensor_arg(t, dtype, shape, name, on_gpu=True):
    """One tensor argument checked against ``dtype`` and ``shape`` (``None``: any size): ``TypeError``, then ``ValueError``.
    With ``on_gpu`` the device is checked between the two and the tensor comes back contiguous; without, the caller does
    both later (:func:`pose_plan`, so that every argument error shows without a GPU)."""
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise TypeError(f"{name} must be a {dtype} tensor")
    if on_gpu:
        require_gpu(t)
    if t.dim() != len(shape) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
        raise ValueError(f"{name} must have shape {tuple('*' if s is None else s for s in shape)}, got {tuple(t.shape)}")
    return t.contiguous() if on_gpu else t


_DTYPES = {torch.float32: _K["OTP_DTYPE_F32"], torch.float16: _K["OTP_DTYPE_F16"], torch.bfloat16: _K["OTP_DTYPE_BF16"],
           torch.float64: _K["OTP_DTYPE_F64"]}

ACT_NONE, ACT_RELU, ACT_GELU = _K["OTP_ACT_NONE"], _K["OTP_ACT_RELU"], _K["OTP_ACT_GELU"]


class View:
    """A channel slice [coff, coff + C) of a contiguous (N, ctot, H, W) float32 tensor."""

    __slots__ = ("t", "coff", "C")

    def __init__(self, t, coff=0, C=None):
        assert t.is_contiguous() and t.dtype == torch.float32 and t.dim() == 4
        self.t, self.coff, self.C = t, coff, (t.shape[1] - coff if C is None else C)
        assert 0 <= coff and coff + self.C <= t.shape[1]

    @property
    def ctot(self):
        return self.t.shape[1]


class H8:
    """An H8 image: ``t`` = int32 storage of [N][gtot][H * W] 16-byte records (8 halves = channels 8 g .. 8 g + 7 of a pixel),
    of which this tensor is the channel groups [goff, goff + C / 8) - the fp16 engine's activation format (include/otpose_hip.h)."""

    __slots__ = ("t", "N", "C", "H", "W", "gtot", "goff")

    def __init__(self, t, n, c, h, w, gtot=None, goff=0):
        assert c % 8 == 0
        self.t, self.N, self.C, self.H, self.W = t, n, c, h, w
        self.gtot, self.goff = (c // 8 if gtot is None else gtot), goff
        assert 0 <= self.goff and self.goff + c // 8 <= self.gtot

    def slice(self, coff, c):
        assert coff % 8 == 0 and c % 8 == 0 and coff + c <= self.C
        return H8(self.t, self.N, c, self.H, self.W, self.gtot, self.goff + coff // 8)


# ---- launch arguments ------------------------------------------------------------------------------------------------------
# One ``*_args`` function per C entry point states its positional arguments (without the trailing stream) once: the eager
# wrappers launch ``fn(*args, stream)`` at once, the inference engine records the same tuple for its launch list.
def _vp(v):
    """Device pointer of the tensor behind a :class:`View` / :class:`H8` (``None`` -> NULL)."""
    return None if v is None else hip.ptr(v.t)


def _slice(v):
    """(total channels, channel offset) of an optional :class:`View` / (groups, group offset) of an :class:`H8`."""
    return (0, 0) if v is None else (v.gtot, v.goff) if isinstance(v, H8) else (v.ctot, v.coff)


def _launch(fn, name, args, t, stream=None):
    """Launch now, on ``stream`` or on the stream PyTorch is enqueuing on for tensor ``t``'s device."""
    hip.check(fn(*args, stream if stream is not None else hip.stream_of(t)), name)
