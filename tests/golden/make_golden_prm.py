#!/usr/bin/env python
"""Generate tests/golden/prm.npz by IMPORTING the reference the way make_golden.py does (build container only).

Run from the repo root:  ``python tests/golden/make_golden_prm.py``

The reference's own ``RSN_ATTENTION`` / ``RSN_WEIGHT_VECTOR`` (model/RSB.py:142-203) in eval mode with randomised running
statistics.  Weights are not stored: both sides regenerate them with ``tests/prm_ref.fill_prm_`` / ``prm_state`` (a seeded rule
for the PRM keys, the synthetic recipe over the key set without them).  Stored per case: the input and the output; the sorted
``state_dict`` key lists and shapes of both classes; and the 7 outputs of one tiny reference ``OTPose`` whose ``def_fuse`` and
``offset_mask_combine_conv`` are each wrapped as ``nn.Sequential(chain, RSN_ATTENTION(c))`` (its ``forward`` untouched)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G                        # noqa: E402  (puts the repo root on sys.path)

from otpose_amd import config as C            # noqa: E402
from otpose_amd import synthetic as S         # noqa: E402
from tests import prm_ref as R                # noqa: E402

# tag -> (class name, constructor arguments, input shape, weight seed, input seed)
CASES = {
    "att_17": ("RSN_ATTENTION", (17,), (2, 17, 5, 7), 31, 41),
    "att_32": ("RSN_ATTENTION", (32,), (1, 32, 13, 19), 32, 42),
    "vec_17_20": ("RSN_WEIGHT_VECTOR", (17, 20), (2, 17, 6, 9), 33, 43),
}
# the wrapped chains of the reference model <-> this package's names (MODEL.PRM)
WRAPPED = {"def_fuse": "def_fuse_prm", "offset_mask_combine_conv": "offset_mask_combine_prm"}


def to_ours(key):
    for chain, prm in WRAPPED.items():
        if key.startswith(chain + ".0."):
            return chain + key[len(chain) + 2:]
        if key.startswith(chain + ".1."):
            return prm + key[len(chain) + 2:]
    return key


def main():
    G.import_reference()
    from model import RSB
    out = {}
    with torch.no_grad():
        for tag, (cls, args, xshape, wseed, xseed) in CASES.items():
            mod = R.fill_prm_(getattr(RSB, cls)(*args), wseed).eval()
            x = G.seeded(xshape, xseed)
            y = mod(x)
            out[tag + "_x"], out[tag + "_y"] = x, y
            print(f"  {tag}: out {tuple(y.shape)} max|.|={y.abs().max():.4g} std={y.std():.4g}")
            sd = mod.state_dict()
            out[tag + "_keys"] = np.array(sorted(sd))
            out[tag + "_shapes"] = np.array([",".join(str(d) for d in sd[k].shape) for k in sorted(sd)])

        cfg = C.tiny_cfg(8, (64, 96))
        m = G.ref_otpose(cfg)
        m.def_fuse = torch.nn.Sequential(m.def_fuse, RSB.RSN_ATTENTION(cfg.MODEL.NUM_JOINTS))
        m.offset_mask_combine_conv = torch.nn.Sequential(m.offset_mask_combine_conv, RSB.RSN_ATTENTION(cfg.MODEL.DEFORMABLE_CONV_CH))
        sd = m.state_dict()
        new = R.prm_state({to_ours(k): tuple(v.shape) for k, v in sd.items()}, S.WEIGHT_SEED, S.gains_for(cfg))
        for k, v in sd.items():
            if to_ours(k) in new:
                v.copy_(new[to_ours(k)].to(v.dtype))
        m.eval()
        x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
        outs = m(x, margin=margin)
        for n, o in zip(("output", "rough", "intersection", "prev_b", "context", "squeezed", "total_b"), outs):
            out["e2e_" + n] = o
            print(f"  {n:13s} max|.|={o.abs().max():.4g} std={o.std():.4g}")
    G.save("prm", **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
