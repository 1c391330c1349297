"""Attention-probability dropout of the three attentions (token: csrc/tokattn.hip, local window: csrc/localattn.hip, channel:
csrc/chanattn.hip): what the callers share, and the mask as a tensor for tests and debugging.

The mask is a counter-based function of (seed, group, row, column, p) - include/otpose_hip.h states it ("attention dropout mask")
- that the forward and the backward kernels evaluate in place; no mask tensor exists on the training path.  The 64-bit seed of a
call comes from PyTorch's CUDA generator (:func:`draw_seed`), so ``torch.manual_seed`` makes a step's masks repeat.  These are
this library's own masks, not the Philox draws PyTorch's dropout would make.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip

__all__ = ["draw_seed", "check_rate", "threshold", "seed_of", "resolve", "keep_mask"]


def draw_seed(device):
    """A 64-bit seed for a counter-based draw from PyTorch's CUDA generator state (seed, Philox offset), advancing the offset like a
    random op does: ``torch.manual_seed`` makes the step's draws repeat, consecutive calls differ.  Host side only."""
    gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
    off = gen.get_offset()
    gen.set_offset(off + 4)
    return (gen.initial_seed() * 0x9E3779B97F4A7C15 + (off + 1) * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF


def check_rate(p, what="dropout_p"):
    """Raise ``ValueError`` unless ``p`` is a real number in [0, 1) whose 16-bit threshold stays below 65536 (a rate of
    1 - 2^-17 or more would drop every entry: the kernels refuse it as well)."""
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what} must be a float in [0, 1), got {p!r}")
    if not (0.0 <= float(p) < 1.0 and threshold(p) < 65536):
        raise ValueError(f"{what} must be in [0, 1 - 2^-17), got {p!r}")
    return float(p)


def threshold(p):
    """``thr`` of the mask definition: ``(uint32)(p * 65536.f + 0.5f)`` in float32; 0 means no dropout."""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def resolve(p, seed, device, what="dropout_p"):
    """(p, seed) of a call: ``p`` validated (:func:`check_rate`), then :func:`seed_of`."""
    return seed_of(check_rate(p, what), seed, device)


def seed_of(p, seed, device):
    """(p, seed) of a call with a validated rate: (0.0, 0) when its threshold is 0 (the plain kernels run), else ``seed`` as a
    64-bit integer, drawn from the CUDA generator when None."""
    if threshold(p) == 0:
        return 0.0, 0
    if seed is None:
        return p, draw_seed(device)
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"seed must be None or an int in [0, 2^64), got {seed!r}")
    return p, int(seed)


def keep_mask(seed, G, R, Ccols, p, device):
    """``(G, R, Ccols)`` uint8, 1 = kept: the mask the attention kernels apply to a probability matrix of G = B * n_head groups,
    R rows and Ccols columns (token: T x T, local: T x window, channel: hs x hs) under ``seed`` and rate ``p``, written by
    ``otp_attn_dropout_keep`` with the kernels' own device function."""
    p = check_rate(p, "p")
    device = torch.device(device)
    if device.type != "cuda":
        raise NotImplementedError("attn_dropout.keep_mask: otpose_amd runs on the GPU only, got device " + str(device))
    if min(int(G), int(R), int(Ccols)) < 1:
        raise ValueError(f"keep_mask: G, R, Ccols must be positive, got {(G, R, Ccols)}")
    out = torch.empty((int(G), int(R), int(Ccols)), dtype=torch.uint8, device=device)
    hip.check(hip.lib().otp_attn_dropout_keep(hip.ptr(out), int(G), int(R), int(Ccols), p, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              hip.stream_of(out)), "otp_attn_dropout_keep")
    return out
