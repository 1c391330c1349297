"""Attention-probability dropout, host side: the statistics of the mask definition (tests/attn_dropout_ref.py restates it in
numpy), the restated attentions against the ones the undropped kernels are held to, the validation of the rates and the ``cfg``
keys, and the declarations of the new entry points.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import attn_dropout_ref as A
from tests import encoder_bwd_ref as E
from tests import local_attn_ref as LR
from tests import token_attn_ref as TR
from tests.conftest import seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 0x123456789ABCDEF, 2 ** 64 - 1]
BIG = (2, 1030, 1030)


def _corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", SEEDS)
def test_kept_share_and_lag_one_correlations(seed, p):
    k = A.keep(seed, *BIG, p)
    assert k.shape == BIG and k.dtype == np.bool_
    q = A.threshold(p) / 65536.0
    n = k.size
    share, sigma = float(k.mean()), math.sqrt(q * (1 - q) / n)
    rows, cols = _corr(k[:, :, 1:], k[:, :, :-1]), _corr(k[:, 1:, :], k[:, :-1, :])
    print(f"ATTNDROP|seed {seed:#x} p {p}|share {share:.6f} expect {1 - q:.6f} ({(share - (1 - q)) / sigma:+.2f} sigma)|"
          f"lag-1 rows {rows:+.5f} cols {cols:+.5f}")
    assert abs(share - (1 - q)) <= 4 * sigma
    assert abs(rows) <= 0.01 and abs(cols) <= 0.01


def test_threshold_and_scale():
    assert A.threshold(0.0) == 0 and A.threshold(0.1) == 6554 and A.threshold(0.5) == 32768 and A.threshold(1e-6) == 0
    assert A.keep_scale(0.5) == 2.0 and A.keep_scale(0.0) == 1.0
    assert bool(A.keep(3, 2, 4, 6, 0.0).all())                                 # thr == 0: nothing is dropped
    from otpose_amd import attn_dropout as D
    for p in (0.0, 1e-6, 0.1, 0.25, 0.5, 0.999):
        assert D.threshold(p) == A.threshold(p)


def test_two_seeds_give_unrelated_masks():
    a, b = A.keep(5, 2, 64, 64, 0.5), A.keep(6, 2, 64, 64, 0.5)
    share = float((a == b).mean())
    assert 0.45 <= share <= 0.55, share
    assert np.array_equal(a, A.keep(5, 2, 64, 64, 0.5))


def _scalar_keep(seed, g, i, j, R, ccols, p):
    """One entry in Python integers, straight from the definition."""
    pair = (g * R + i) * ((ccols + 1) // 2) + (j >> 1)
    m = 0xFFFFFFFF
    h = ((pair & m) * 0x9E3779B1 + (seed & m)) & m
    h ^= (((pair >> 32) + (seed >> 32)) & m) * 0x85EBCA77 & m
    h ^= h >> 16
    h = h * 0x21F0AAAD & m
    h ^= h >> 15
    h = h * 0x735A2D97 & m
    h ^= h >> 15
    return ((h >> 16) if j & 1 else (h & 0xFFFF)) >= A.threshold(p)


@pytest.mark.parametrize("shape", [(3, 5, 5), (2, 7, 33), (2, 6, 4), (1, 3, 1)])
def test_odd_and_even_column_counts_match_the_scalar_definition(shape):
    G, R, C = shape
    for seed in (0x123456789ABCDEF, 2 ** 64 - 1):
        k = A.keep(seed, G, R, C, 0.5)
        want = np.array([[[_scalar_keep(seed, g, i, j, R, C, 0.5) for j in range(C)] for i in range(R)] for g in range(G)])
        assert np.array_equal(k, want)
    # a row's pairs do not run into the next row's: with an odd count the last pair's high half is unused
    assert np.array_equal(A.keep(9, 1, 4, 5, 0.5)[0, :, :4], A.keep(9, 1, 4, 6, 0.5)[0, :, :4])


def test_pair_index_beyond_32_bits():
    pair = np.array([2 ** 32 + 5, 5], dtype=np.uint64)
    h = A.drop_hash(pair, 7)
    assert h[0] != h[1]


def test_the_named_dropped_row_case():
    k = A.keep(0x123456789ABCDEF, 1, 5, 5, 0.5)
    dead = [i for i in range(5) if not k[0, i].any()]
    assert len(dead) == 1, k


def test_restatements_with_an_all_ones_mask_equal_the_undropped_ones():
    D = torch.float64
    q, k, v = (seeded((2, 34, 12), 50 + i).to(D) for i in range(3))
    mask = torch.zeros(2, 12, dtype=torch.bool)
    mask[1, 3] = True
    assert torch.equal(A.token_attn(q, k, v, 2, 0.3, A.ones(4, 12, 12), mask), TR.token_attn(q, k, v, 2, 0.3, mask))
    rel = seeded((1, 1, 2, 5), 60, 0.5).to(D)
    q, k, v = (seeded((2, 34, 8), 70 + i).to(D) for i in range(3))
    assert torch.equal(A.local_attn(q, k, v, 2, 5, 0.3, A.ones(4, 8, 5), rel), LR.local_attn(q, k, v, 2, 5, 0.3, rel))
    assert torch.equal(A.chan_attn(q, k, v, 2, 0.3, A.ones(4, 17, 17)), E.chan_attn_expr(q, k, v, 2, 0.3))


def test_restated_dropout_scales_survivors():
    """p = 0.5 on a uniform attention (q = 0): every output is the sum over the surviving keys of 2 / T times v."""
    D = torch.float64
    t = 6
    v = seeded((1, 3, t), 5).to(D)
    z = torch.zeros_like(v)
    m = A.factors(11, 1, t, t, 0.5)
    want = torch.einsum("ij,cj->ci", m[0] / t, v[0])
    assert torch.allclose(A.token_attn(z, z, v, 1, 1.0, m)[0], want, atol=1e-15)
    assert set(m.unique().tolist()) <= {0.0, 2.0}


def test_rate_validation():
    from otpose_amd import attn_dropout as D
    from otpose_amd import modules as M
    from otpose_amd import token_attn as TA
    from otpose_amd import train_ops as T
    for bad in (-0.1, 1.0, 1.5, float("nan"), "0.1", None, True, 1 - 1e-9, 1 - 2.0 ** -17, 1 - 2.0 ** -18):
        with pytest.raises(ValueError):
            D.check_rate(bad)
    assert D.check_rate(0) == 0.0 and D.check_rate(0.999) == 0.999
    assert D.threshold(1 - 2.0 ** -16) == 65535 and D.check_rate(1 - 2.0 ** -16) == 1 - 2.0 ** -16      # the largest threshold
    x = torch.zeros(1, 4, 4)
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="dropout_p"):
            TA.token_attn(x, x, x, 1, 1.0, dropout_p=bad)
        with pytest.raises(ValueError, match="dropout_p"):
            T.chan_attn(x, x, x, 1, 1.0, dropout_p=bad)
        with pytest.raises(ValueError, match="dropout_p"):
            T.local_attn(x, x, x, 1, 5, 1.0, dropout_p=bad)
        with pytest.raises(ValueError, match="attn_dropout"):
            M.TransformerEncoderLayer(136, 2, 272, attn_dropout=bad)
    with pytest.raises(ValueError, match="seed"):
        D.resolve(0.5, -1, torch.device("cpu"))
    assert D.resolve(1e-6, None, torch.device("cpu")) == (0.0, 0)               # threshold 0: nothing is drawn
    with pytest.raises(NotImplementedError):
        D.keep_mask(1, 1, 2, 2, 0.5, "cpu")


def test_encoder_layer_takes_attention_dropout():
    """The constructor argument stays refused (tests/test_token_attn_host.py pins that); a built layer takes the rate."""
    from otpose_amd import modules as M
    layer = M.TransformerEncoderLayer(136, 2, 272)
    assert layer.attn_dropout == 0.0 and layer.p_drop == 0.1                    # `dropout` alone behaves as before
    assert layer.set_attn_dropout(0.1) is layer and layer.attn_dropout == 0.1
    enc = M.TransformerEncoder(layer, 2)
    assert [lyr.attn_dropout for lyr in enc.layers] == [0.1, 0.1]
    for bad in (-0.1, 1.0, "0.1", None):
        with pytest.raises(ValueError, match="attn_dropout"):
            layer.set_attn_dropout(bad)
    assert layer.attn_dropout == 0.1


def _keyed_cfg(**keys):
    from otpose_amd import tiny_cfg
    cfg = tiny_cfg(8, (64, 96))
    for k, v in keys.items():
        cfg.MODEL[k] = v
    return cfg


def test_cfg_keys_reach_the_modules_and_change_no_parameter():
    from otpose_amd import OTPose, tiny_cfg
    from otpose_amd import modules as M
    base = OTPose(tiny_cfg(8, (64, 96)))
    assert all(m.attn_pdrop == 0.0 for m in base.modules() if isinstance(m, M.MaskedMHCA))
    m = OTPose(_keyed_cfg(ATTN_PDROP=0.1, FLOW_ATTN_PDROP=0.2, TOKEN_ATTN_DROPOUT=0.3, TOKEN_LAYERS=1, FLOW_TOKEN_LAYERS=1))
    rates = lambda enc: {a.attn_pdrop for a in enc.modules() if isinstance(a, M.MaskedMHCA)}      # noqa: E731
    assert rates(m.temporal_encoder1) == {0.1} and rates(m.temporal_encoder2) == {0.1} and rates(m.flow_encoder) == {0.2}
    for name in ("token_encoder1", "token_encoder2", "flow_token_encoder"):
        assert [lyr.attn_dropout for lyr in getattr(m, name).layers] == [0.3]
    plain = OTPose(_keyed_cfg(TOKEN_LAYERS=1, FLOW_TOKEN_LAYERS=1))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in plain.state_dict().items()}
    # a windowed encoder cannot train with a rate (TrainGraph.attention still refuses it): the pair of keys is refused by name
    with pytest.raises(ValueError, match="ATTN_PDROP.*MHA_WIN_SIZE"):
        OTPose(_keyed_cfg(MHA_WIN_SIZE=[9, 9, 9], ATTN_PDROP=0.1))
    with pytest.raises(ValueError, match="FLOW_ATTN_PDROP.*FLOW_MHA_WIN_SIZE"):
        OTPose(_keyed_cfg(FLOW_MHA_WIN_SIZE=9, FLOW_ATTN_PDROP=0.1))
    OTPose(_keyed_cfg(MHA_WIN_SIZE=[9, 9, 9], FLOW_ATTN_PDROP=0.1))             # the flow encoder keeps the channel attention


@pytest.mark.parametrize("key", ["ATTN_PDROP", "FLOW_ATTN_PDROP", "TOKEN_ATTN_DROPOUT"])
@pytest.mark.parametrize("value", [-0.1, 1.0, "0.1", None, True])
def test_cfg_keys_are_validated(key, value):
    from otpose_amd import OTPose
    with pytest.raises(ValueError, match=key):
        OTPose(_keyed_cfg(**{key: value}))


def test_the_inference_engines_read_none_of_the_keys():
    for name in ("engine.py", "engine_h16.py"):
        src = open(os.path.join(ROOT, "otpose_amd", name)).read()
        for word in ("ATTN_PDROP", "TOKEN_ATTN_DROPOUT", "attn_pdrop", "attn_dropout"):
            assert word not in src, (name, word)


def test_the_bf16_training_graph_inherits_attention():
    from otpose_amd import train as TRN
    assert "attention" not in vars(TRN.TrainGraphBF16) and TRN.TrainGraphBF16.attention is TRN.TrainGraph.attention


NEW_SYMBOLS = ("otp_attn_dropout_keep", "otp_token_attn_forward_dropout", "otp_token_attn_backward_dropout",
               "otp_local_attn_dropout", "otp_local_attn_backward_dropout", "otp_chan_attn_dropout_workspace",
               "otp_chan_attn_dropout", "otp_softmax_backward_dropout")


def test_new_entry_points_are_declared_bound_and_check_their_arguments():
    from ctypes import c_float, c_ulonglong
    from otpose_amd import hip
    src = open(os.path.join(ROOT, "include", "otpose_hip.h")).read()
    assert "attention dropout mask" in src
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", src), name
        assert name in hip.SIGNATURES
        if name != "otp_chan_attn_dropout_workspace":
            assert hip.SIGNATURES[name][1][-3:-1] == [c_float, c_ulonglong], name
    L = hip.lib()
    assert L.otp_attn_dropout_keep(None, 1, 1, 1, 0.5, 1, None) == -1
    one = (ctypes.c_ubyte * 4)()                                               # a rate is refused before any launch: host memory will do
    for bad in (-0.1, 1.0, 1 - 2.0 ** -17, float("nan")):                        # 1 - 2^-17: its threshold would be 65536
        assert L.otp_attn_dropout_keep(ctypes.cast(one, ctypes.c_void_p), 1, 2, 2, bad, 1, None) == -1, bad
    assert L.otp_token_attn_forward_dropout(None, None, None, None, None, None, 1, 4, 1, 4, 1.0, 0.5, 1, None) == -1
    assert L.otp_chan_attn_dropout_workspace(2, 136, 100, 2) == L.otp_chan_attn_workspace(2, 136, 100, 2) + 4 * 80 * 80 * 4
    assert L.otp_chan_attn_dropout_workspace(2, 135, 100, 2) == 0
    # one copy of the hash: csrc/common.h
    csrc = os.path.join(ROOT, "otpose_amd", "csrc")
    holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip"))
               and re.search(r"uint32_t\s+otp_drop_hash\s*\(", open(os.path.join(csrc, f)).read())]
    assert holders == ["common.h"]
