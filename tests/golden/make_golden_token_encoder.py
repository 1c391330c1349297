#!/usr/bin/env python
"""Generate tests/golden/token_encoder.npz by IMPORTING the reference the way make_golden.py does (build container only).

Run from the repo root:  ``python tests/golden/make_golden_token_encoder.py``

The reference's own ``TransformerEncoder`` / ``TransformerEncoderLayer`` (model/OTPose.py:26-159) in eval mode and its
``_make_sine_position_embedding`` (:281-305, called on a stand-in object that carries ``pe_h`` / ``pe_w``).  Weights are not
stored: both sides regenerate them with ``tests/token_attn_ref.fill_encoder_``.  Stored per case: the input, ``pos``, the key
padding mask, the output, the attention maps where the case asks for them, and the sorted ``state_dict`` key and shape lists."""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G                        # noqa: E402  (puts the repo root on sys.path)

from tests import token_attn_ref as R         # noqa: E402

# tag -> (E, heads, FFN, activation, pre-norm, layers, final norm, pe_only_at_begin, maps, L or (h, w), N, masked keys per sample)
CASES = {
    "a": (136, 2, 272, "gelu", False, 2, False, False, False, (12, 9), 2, None),
    "b": (17, 1, 34, "relu", True, 2, True, False, True, 35, 2, (3, 11)),
    "c": (136, 2, 272, "gelu", False, 2, False, True, False, (12, 9), 2, None),
}
SINE = [(12, 9, 136), (5, 7, 8), (16, 12, 204)]
WEIGHT_SEED, INPUT_SEED = {"a": 10, "b": 40, "c": 10}, {"a": 1, "b": 2, "c": 1}


def masked_keys(tag, n, length, counts):
    """(N, L) bool with counts[i] True entries in sample i, at seeded positions; at least one key stays live."""
    mask = torch.zeros(n, length, dtype=torch.bool)
    for i, cnt in enumerate(counts):
        g = torch.Generator().manual_seed(500 + 7 * i + len(tag))
        mask[i, torch.randperm(length, generator=g)[:cnt]] = True
    return mask


def main():
    G.import_reference()
    from model import OTPose as RO
    out = {}

    def sine(h, w, d):
        return RO.OTPose._make_sine_position_embedding(types.SimpleNamespace(pe_h=h, pe_w=w), d)

    with torch.no_grad():
        for tag, (e, nh, ffn, act, pre, layers, norm, pe_begin, maps, grid, n, nmask) in CASES.items():
            layer = RO.TransformerEncoderLayer(e, nh, ffn, activation=act, normalize_before=pre, return_atten_map=maps)
            enc = RO.TransformerEncoder(layer, layers, torch.nn.LayerNorm(e) if norm else None, pe_begin, maps)
            R.fill_encoder_(enc, WEIGHT_SEED[tag]).eval()
            if isinstance(grid, tuple):
                length = grid[0] * grid[1]
                pos = sine(grid[0], grid[1], e).permute(1, 0, 2)                  # (L, 1, E), as OTPose.forward hands it over
            else:
                length = grid
                pos = G.seeded((length, 1, e), 60 + INPUT_SEED[tag], 0.5)
            src = G.seeded((length, n, e), INPUT_SEED[tag])
            mask = masked_keys(tag, n, length, nmask) if nmask else None
            res = enc(src, src_key_padding_mask=mask, pos=pos)
            y, amaps = res if maps else (res, None)
            out[tag + "_x"], out[tag + "_pos"], out[tag + "_y"] = src, pos, y
            if mask is not None:
                out[tag + "_mask"] = mask
            if amaps is not None:
                out[tag + "_maps"] = amaps
            sd = enc.state_dict()
            out[tag + "_keys"] = np.array(sorted(sd))
            out[tag + "_shapes"] = np.array([",".join(str(d) for d in sd[k].shape) for k in sorted(sd)])
            lsd = layer.state_dict()
            out[tag + "_layer_keys"] = np.array(sorted(lsd))
            out[tag + "_layer_shapes"] = np.array([",".join(str(d) for d in lsd[k].shape) for k in sorted(lsd)])
            print(f"  {tag}: out {tuple(y.shape)} max|.|={y.abs().max():.4g} std={y.std():.4g}")
        for h, w, d in SINE:
            out[f"sine_{h}_{w}_{d}"] = sine(h, w, d)
    G.save("token_encoder", **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
