"""Heat-map decode, flip-test merge and PCK (csrc/glue.hip)."""
from __future__ import annotations

import ctypes

import torch

from .. import hip
from ..augment import FLIP_PAIRS
from .base import check_f32, require_gpu


def get_max_preds(batch_heatmaps):
    """Device form of reference utils/heatmap.py:143-171: (N,J,H,W) heat-maps -> (preds (N,J,2), maxvals (N,J,1)),
    no device-to-host copy of the maps."""
    return _decode(batch_heatmaps, None, None, refine=False)


def get_final_preds(batch_heatmaps, center=None, scale=None):
    """Device form of reference utils/heatmap.py:108-132: argmax, +-0.25 px shift towards the higher neighbour, and
    (when ``center`` / ``scale`` (N,2) are given) the rot = 0 inverse crop transform of transform_preds."""
    return _decode(batch_heatmaps, center, scale, refine=True)


def _decode(hm, center, scale, refine):
    require_gpu(hm)
    check_f32(hm)
    if hm.dim() != 4:
        raise AssertionError("batch_images should be 4-ndim")
    hm = hm.contiguous()
    n, j, h, w = hm.shape
    preds = torch.empty((n, j, 2), dtype=torch.float32, device=hm.device)
    maxvals = torch.empty((n, j, 1), dtype=torch.float32, device=hm.device)
    c = s_ = None
    if center is not None:
        c = torch.as_tensor(center, dtype=torch.float32, device=hm.device).reshape(n, 2).contiguous()
        s_ = torch.as_tensor(scale, dtype=torch.float32, device=hm.device).reshape(n, 2).contiguous()
    hip.check(hip.lib().otp_heatmap_decode(hip.ptr(hm), hip.ptr(preds), hip.ptr(maxvals), hip.ptr(c), hip.ptr(s_),
                                           n, j, h, w, int(refine), hip.stream_of(hm)), "otp_heatmap_decode")
    return preds, maxvals


def flip_permutation(pairs, num_joints):
    """The involution of the left/right ``pairs`` over ``num_joints`` joints as an int32 numpy array (unpaired joints map
    to themselves) - what HRNet's ``flip_back`` swaps.  Host only; raises ``ValueError`` for a joint outside
    [0, num_joints) or one that appears twice (the pairs would not be an involution)."""
    import numpy as np
    j = int(num_joints)
    if j <= 0:
        raise ValueError("num_joints must be positive")
    perm = np.arange(j, dtype=np.int32)
    seen = set()
    for pair in pairs:
        if len(pair) != 2:
            raise ValueError(f"flip pair {pair!r} is not a pair")
        a, b = (int(v) for v in pair)
        for v in (a, b):
            if not 0 <= v < j:
                raise ValueError(f"flip pair {pair!r}: joint {v} outside [0, {j})")
            if v in seen:
                raise ValueError(f"flip pairs: joint {v} appears twice (not an involution)")
            seen.add(v)
        perm[a], perm[b] = b, a
    return perm


def flip_test_merge(hm_pair, flip_pairs=FLIP_PAIRS, shift_heatmap=False, center=None, scale=None):
    """Flip test of HRNet's ``validate`` (TEST.FLIP_TEST / TEST.SHIFT_HEATMAP) in one kernel: ``hm_pair`` (2B, J, H, W)
    float32 are the heat-maps of one forward over the plain clips ``[:B]`` and their mirrors ``[B:]`` (:func:`mirror_pair`,
    ``crop_clips(mirror_pair=True)``).  The mirrored maps are flipped back with the left/right joints of ``flip_pairs``
    (``augment.FLIP_PAIRS``: PoseTrack's 17 joints) swapped, shifted one column right under ``shift_heatmap``, and averaged with the plain
    maps as ``(a + b) * 0.5`` in float32; ``get_final_preds`` of the result comes out of the same pass.  Returns
    ``(merged (B, J, H, W), preds (B, J, 2), maxvals (B, J, 1))``; ``center`` / ``scale`` (B, 2) as for
    :func:`get_final_preds`."""
    require_gpu(hm_pair)
    check_f32(hm_pair)
    if hm_pair.dim() != 4 or hm_pair.shape[0] % 2:
        raise ValueError("hm_pair must be a (2B, J, H, W) tensor")
    hm_pair = hm_pair.contiguous()
    n2, j, h, w = hm_pair.shape
    n = n2 // 2
    perm = flip_permutation(flip_pairs, j)
    merged = torch.empty((n, j, h, w), dtype=torch.float32, device=hm_pair.device)
    preds = torch.empty((n, j, 2), dtype=torch.float32, device=hm_pair.device)
    maxvals = torch.empty((n, j, 1), dtype=torch.float32, device=hm_pair.device)
    c = s_ = None
    if (center is None) != (scale is None):
        raise ValueError("center and scale go together")
    if center is not None:
        c = torch.as_tensor(center, dtype=torch.float32, device=hm_pair.device).reshape(n, 2).contiguous()
        s_ = torch.as_tensor(scale, dtype=torch.float32, device=hm_pair.device).reshape(n, 2).contiguous()
    hip.check(hip.lib().otp_heatmap_flip_decode(hip.ptr(hm_pair), perm.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), hip.ptr(merged),
                                                hip.ptr(preds), hip.ptr(maxvals), hip.ptr(c), hip.ptr(s_), n, j, h, w,
                                                int(bool(shift_heatmap)), hip.stream_of(hm_pair)),
              "otp_heatmap_flip_decode")
    return merged, preds, maxvals


def mirror_pair(x, out=None):
    """The flip-test twin batch of clips that are already normalised: ``x`` (B, C, H, W) float32 -> (2B, C, H, W) with
    ``[:B] = x`` and ``[B:] = x.flip(3)`` (script/Common.py:348-354), one streaming kernel.  ``out`` is written in place."""
    require_gpu(x)
    check_f32(x)
    if x.dim() != 4:
        raise ValueError("x must be a (B, C, H, W) tensor")
    x = x.contiguous()
    b, c, h, w = x.shape
    if out is None:
        out = torch.empty((2 * b, c, h, w), dtype=torch.float32, device=x.device)
    elif (tuple(out.shape) != (2 * b, c, h, w) or out.dtype != torch.float32 or not out.is_contiguous()
          or out.device != x.device):
        raise ValueError("out must be a contiguous float32 (2B, C, H, W) tensor on x's device")
    hip.check(hip.lib().otp_clip_mirror_pair(hip.ptr(x), hip.ptr(out), b, c, h, w, hip.stream_of(x)),
              "otp_clip_mirror_pair")
    return out


def accuracy(output, target, hm_type="gaussian", thr=0.5):
    """Device form of reference utils/evaluate.py:384-415 (called per iteration at script/Common.py:147-150 on heat-maps
    copied to the host): PCK of the argmax of ``output`` against the argmax of ``target``.  Returns
    ``(acc (J+1), avg_acc, cnt, pred)`` like the reference, as device tensors (no synchronisation)."""
    if hm_type != "gaussian":
        raise NotImplementedError("only hm_type='gaussian' (the reference's only caller)")
    pred, _ = get_max_preds(output)
    tgt, _ = get_max_preds(target)
    n, j, h, w = output.shape
    acc = torch.empty(j + 1, dtype=torch.float32, device=output.device)
    cnt = torch.empty(1, dtype=torch.int32, device=output.device)
    hip.check(hip.lib().otp_pck_accuracy(hip.ptr(pred), hip.ptr(tgt), hip.ptr(acc), hip.ptr(cnt), n, j, h, w, float(thr),
                                         hip.stream_of(output)), "otp_pck_accuracy")
    return acc, acc[0], cnt[0], pred
