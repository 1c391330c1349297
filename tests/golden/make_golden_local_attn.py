#!/usr/bin/env python
"""Generate tests/golden/local_attn.npz by IMPORTING the reference the way make_golden.py does (build container only).

Run from the repo root:  ``python tests/golden/make_golden_local_attn.py``

The reference's own ``LocalMaskedMHCA`` / ``TransformerBlock`` / ``ConvTransformer`` / ``OTPose`` in eval mode with a local
attention window.  Weights are not stored: both sides regenerate them with ``tests/local_attn_ref.fill_windowed_`` (the synthetic
recipe over the key set without ``rel_pe``) - except every ``rel_pe``, which is drawn with ``seeded()`` here and STORED, so the
recipe needs no rule for it.  Stored per case: the input, the output(s), the rel_pe tensors; plus the sorted ``state_dict`` key
list of the windowed TransformerBlock.  The tiny OTPose regenerates its clip from ``synthetic.synthetic_clip``."""
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
from tests import local_attn_ref as R         # noqa: E402

REL_SEED = 900          # rel_pe of the i-th rel_pe key (sorted) of a module: seeded(shape, REL_SEED + i, REL_STD)
REL_STD = 0.2


def rel_pes(module):
    keys = sorted(k for k in module.state_dict() if k.rsplit(".", 1)[-1] == "rel_pe")
    return {k: G.seeded(tuple(module.state_dict()[k].shape), REL_SEED + i, REL_STD) for i, k in enumerate(keys)}


def fill(module, seed, gains=None):
    rel = rel_pes(module)
    R.fill_windowed_(module, seed, rel, gains)
    return module.eval(), rel


def main():
    G.import_reference()
    from model.blocks import LocalMaskedMHCA, TransformerBlock
    from model.ConvVideoTransformer import ConvTransformer
    out = {}

    def put_rel(tag, rel):
        for k, v in rel.items():
            out[f"{tag}_rel/{k}"] = v

    with torch.no_grad():
        # (C, n_head, window, stride, B, T)
        for tag, (c, nh, win, stride, b, t) in {"lmhca_136_s1": (136, 2, 9, 1, 1, 96), "lmhca_136_s2": (136, 2, 9, 2, 1, 96),
                                                "lmhca_17_s1": (17, 1, 5, 1, 2, 48)}.items():
            mod, rel = fill(LocalMaskedMHCA(c, nh, win, n_qx_stride=stride, n_kv_stride=stride, proj_pdrop=0.1,
                                            use_rel_pe=True), 11)
            x = G.seeded((b, c, t), 21)
            out[tag + "_x"], out[tag + "_y"] = x, mod(x)
            put_rel(tag, rel)
        for tag, (c, nh, stride, b) in {"ltblock_136_s1": (136, 2, 1, 1), "ltblock_136_s2": (136, 2, 2, 1),
                                        "ltblock_17_s1": (17, 1, 1, 2)}.items():
            mod, rel = fill(TransformerBlock(c, nh, n_ds_strides=(stride, stride), attn_pdrop=0.1, proj_pdrop=0.1,
                                             path_pdrop=0.1, mha_win_size=9, use_rel_pe=True), 12)
            x = G.seeded((b, c, 96), 22)
            out[tag + "_x"], out[tag + "_y"] = x, mod(x)
            put_rel(tag, rel)
            if tag == "ltblock_136_s1":
                out["ltblock_keys"] = np.array(sorted(mod.state_dict()))
        mod, rel = fill(ConvTransformer(136, 136, n_head=2, n_embd_ks=3, max_len=96, arch=(0, 2, 2), mha_win_size=[9, 9, 5],
                                        use_rel_pe=True, proj_pdrop=0.1, path_pdrop=0.1, h=12), 14)
        x = G.seeded((1, 136, 12, 8), 24)
        out["lct_136_x"] = x
        for i, y in enumerate(mod(x)):
            out[f"lct_136_y{i}"] = y
        put_rel("lct_136", rel)

        # tiny OTPose with both temporal encoders rebuilt with a window of 9 and rel_pe (T = 384 / 192 / 96)
        cfg = C.tiny_cfg(8, (64, 96))
        m = G.ref_otpose(cfg)
        d = m.temporal_encoding_dim
        for name in ("temporal_encoder1", "temporal_encoder2"):
            setattr(m, name, ConvTransformer(d, d, n_head=2, n_embd_ks=3, max_len=m.num_patches, arch=m.scale_arch,
                                             proj_pdrop=0.1, path_pdrop=0.1, h=m.pe_h, mha_win_size=9, use_rel_pe=True))
        m, rel = fill(m, S.WEIGHT_SEED, S.gains_for(cfg))
        x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
        outs = m(x, margin=margin)
        for n, o in zip(("output", "rough", "intersection", "prev_b", "context", "squeezed", "total_b"), outs):
            out["e2e_" + n] = o
            print(f"  {n:13s} max|.|={o.abs().max():.4g} std={o.std():.4g}")
        put_rel("e2e", rel)
    G.save("local_attn", **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
