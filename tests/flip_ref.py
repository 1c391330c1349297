"""numpy restatement of the flip test (csrc/glue.hip otp_heatmap_flip_decode, include/otpose_hip.h): HRNet's flip_back,
the optional one-column shift and the float32 average, then get_final_preds with the decode kernel's rules.

``hrnet_flip_merge`` transcribes HRNet's ``validate`` + ``flip_back`` literally (the loop over the pairs, the in-place
shift) and is what ``flip_merge`` is checked against."""
from __future__ import annotations

import numpy as np


def flip_merge(hm_pair, perm, shift):
    """merged (B, J, H, W) float32 of hm_pair (2B, J, H, W): (hm[b] + S[b]) * 0.5 with S the flipped-back mirror maps."""
    hm = np.asarray(hm_pair, np.float32)
    b = hm.shape[0] // 2
    f = hm[b:][:, np.asarray(perm)][..., ::-1]
    s = f.copy()
    if shift:
        s[..., 1:] = f[..., :-1]
    return ((hm[:b] + s) * np.float32(0.5)).astype(np.float32)


def hrnet_flip_back(output_flipped, matched_parts):
    """HRNet lib/utils/transforms.py flip_back (target_type gaussian), as written there."""
    assert output_flipped.ndim == 4
    output_flipped = output_flipped[:, :, :, ::-1]
    for pair in matched_parts:
        tmp = output_flipped[:, pair[0], :, :].copy()
        output_flipped[:, pair[0], :, :] = output_flipped[:, pair[1], :, :]
        output_flipped[:, pair[1], :, :] = tmp
    return output_flipped


def hrnet_flip_merge(output, output_flipped, flip_pairs, shift):
    """HRNet lib/core/function.py validate: flip_back, `output_flipped[:, :, :, 1:] = output_flipped.clone()[:, :, :, 0:-1]`
    under SHIFT_HEATMAP, then `(output + output_flipped) * 0.5`."""
    output_flipped = hrnet_flip_back(np.array(output_flipped, np.float32), flip_pairs).copy()
    if shift:
        output_flipped[:, :, :, 1:] = output_flipped.copy()[:, :, :, 0:-1]
    return (np.asarray(output, np.float32) + output_flipped) * np.float32(0.5)


def _quarter(d):
    """np.sign(d) * .25, with a NaN difference moving nothing (as the kernel)."""
    return np.float32(0.25) if d > 0 else (np.float32(-0.25) if d < 0 else np.float32(0.0))


def final_preds(hm):
    """get_final_preds without the crop transform, with otp_heatmap_decode's rules: the first maximum (the first NaN
    when there is one), the maxvals > 0 mask, the +-0.25 refinement under the strict 1 < p < size - 1 bounds.
    Returns (preds (N, J, 2), maxvals (N, J, 1)) float32."""
    hm = np.asarray(hm, np.float32)
    n, j, h, w = hm.shape
    flat = hm.reshape(n, j, h * w)
    preds = np.zeros((n, j, 2), np.float32)
    maxvals = np.zeros((n, j, 1), np.float32)
    for a in range(n):
        for k in range(j):
            row = flat[a, k]
            nan = np.isnan(row)
            idx = int(np.argmax(nan)) if nan.any() else int(np.argmax(row))
            v = row[idx]
            m = np.float32(1.0) if v > 0 else np.float32(0.0)
            x, y = np.float32(idx % w) * m, np.float32(idx // w) * m
            px, py = int(np.floor(x + 0.5)), int(np.floor(y + 0.5))
            if 1 < px < w - 1 and 1 < py < h - 1:
                p = hm[a, k]
                x = np.float32(x + _quarter(p[py, px + 1] - p[py, px - 1]))
                y = np.float32(y + _quarter(p[py + 1, px] - p[py - 1, px]))
            preds[a, k] = (x, y)
            maxvals[a, k, 0] = v
    return preds, maxvals
