#!/usr/bin/env python
"""Generate tests/golden/conv_embd.npz by IMPORTING the reference the way make_golden.py does (build container only).

Run from the repo root:  ``python tests/golden/make_golden_conv_embd.py``

The reference's own ``ConvTransformer`` / ``OTPose`` in eval mode with conv embedding layers (``arch[0] > 0``).  Weights are not
stored: both sides regenerate them with ``tests/conv_embd_ref.fill_embd_`` (the synthetic recipe over the key set without the
embedding keys, a seeded rule for those).  Stored per case: the input and the outputs; plus the sorted ``state_dict`` key lists
and shapes of the first and third case.  The tiny OTPose regenerates its clip from ``synthetic.synthetic_clip``."""
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
from tests import conv_embd_ref as R          # noqa: E402

# tag -> (constructor arguments, keyword arguments, input shape, weight seed, input seed)
CASES = {
    "ct_136": ((136, 136), dict(n_head=2, n_embd_ks=3, max_len=96, arch=(2, 1, 1), h=12), (1, 136, 12, 8), 15, 25),
    "ct_17": ((17, 17, 1, 3, 48), dict(arch=(1, 1, 0), h=8), (2, 17, 8, 6), 16, 26),
    "ct_24_40": ((24, 40, 2, 5, 35), dict(arch=(2, 1, 0), h=7, with_ln=False), (1, 24, 7, 5), 17, 27),
}


def main():
    G.import_reference()
    from model.ConvVideoTransformer import ConvTransformer
    out = {}
    with torch.no_grad():
        for tag, (args, kw, xshape, wseed, xseed) in CASES.items():
            mod = R.fill_embd_(ConvTransformer(*args, **kw), wseed).eval()
            x = G.seeded(xshape, xseed)
            out[tag + "_x"] = x
            for i, y in enumerate(mod(x)):
                out[f"{tag}_y{i}"] = y
                print(f"  {tag} level {i}: max|.|={y.abs().max():.4g} std={y.std():.4g}")
            if tag in ("ct_136", "ct_24_40"):
                sd = mod.state_dict()
                out[tag + "_keys"] = np.array(sorted(sd))
                out[tag + "_shapes"] = np.array([",".join(str(d) for d in sd[k].shape) for k in sorted(sd)])

        # tiny OTPose with both temporal encoders rebuilt with one conv embedding layer
        cfg = C.tiny_cfg(8, (64, 96))
        m = G.ref_otpose(cfg)
        d = m.temporal_encoding_dim
        for name in ("temporal_encoder1", "temporal_encoder2"):
            setattr(m, name, ConvTransformer(d, d, n_head=2, n_embd_ks=3, max_len=m.num_patches, arch=(1, 6, 2),
                                             proj_pdrop=0.1, path_pdrop=0.1, h=m.pe_h))
        m = R.fill_embd_(m, S.WEIGHT_SEED, S.gains_for(cfg)).eval()
        x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
        outs = m(x, margin=margin)
        for n, o in zip(("output", "rough", "intersection", "prev_b", "context", "squeezed", "total_b"), outs):
            out["e2e_" + n] = o
            print(f"  {n:13s} max|.|={o.abs().max():.4g} std={o.std():.4g}")
    G.save("conv_embd", **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
