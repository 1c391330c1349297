"""Conv embedding of ConvTransformer on the CPU: tests/conv_embd_ref.py against the reference's own classes
(tests/golden/conv_embd.npz), the parameter containers' key sets and shapes, the cfg keys and their validation, the optimizer
grouping of the new parameters, and the argument checks of the C entry points (which return before touching a GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from otpose_amd import OTPose, hip, tiny_cfg
from otpose_amd import modules as M
from otpose_amd import optim
from tests import conv_embd_ref as R

TOL = 1e-5      # restatement vs reference, relative to max(1, max|ref|)

# tag -> (positional, keyword arguments of ConvTransformer, n_head, weight seed): the cases of tests/golden/make_golden_conv_embd.py
CASES = {
    "ct_136": ((136, 136, 2, 3, 96), dict(arch=(2, 1, 1), h=12), 2, 15),
    "ct_17": ((17, 17, 1, 3, 48), dict(arch=(1, 1, 0), h=8), 1, 16),
    "ct_24_40": ((24, 40, 2, 5, 35), dict(arch=(2, 1, 0), h=7, with_ln=False), 2, 17),
}


def build_case(tag):
    args, kw, n_head, seed = CASES[tag]
    ct = R.fill_embd_(M.ConvTransformer(*args, **kw), seed)
    return ct, n_head, kw["arch"]


def _close(got, ref, tol=TOL):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = float((got - ref).abs().max())
    assert err <= tol * max(1.0, float(ref.abs().max())), err


def _raw(name="conv_embd"):
    return np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))


@pytest.mark.parametrize("tag", sorted(CASES))
def test_restatement_matches_reference_conv_transformer(golden, tag):
    g = golden("conv_embd")
    ct, n_head, arch = build_case(tag)
    sd = {"c." + k: v.detach() for k, v in ct.state_dict().items()}
    outs = R.conv_transformer(sd, "c", g[tag + "_x"], n_head, arch)
    assert len(outs) == arch[2] + 1
    for i, y in enumerate(outs):
        _close(y, g[f"{tag}_y{i}"].reshape(y.shape))


@pytest.mark.parametrize("tag", ["ct_136", "ct_24_40"])
def test_containers_own_the_reference_keys_and_shapes(tag):
    z = _raw()
    want = [str(k) for k in z[tag + "_keys"]]
    shapes = [tuple(int(d) for d in str(s).split(",")) for s in z[tag + "_shapes"]]
    ct, _, _ = build_case(tag)
    sd = ct.state_dict()
    assert sorted(sd) == want
    assert [tuple(sd[k].shape) for k in want] == shapes


def test_embedding_layers_follow_with_ln():
    ct = M.ConvTransformer(24, 40, 2, 5, 35, (2, 1, 0), h=7)
    assert [tuple(c.weight.shape) for c in ct.embd] == [(40, 24, 5, 5), (40, 40, 5, 5)]
    assert all(c.bias is None and c.padding == (2, 2) for c in ct.embd)
    assert all(type(n) is M.LayerNorm and tuple(n.weight.shape) == (1, 40, 1) for n in ct.embd_norm)
    ct = M.ConvTransformer(24, 40, 2, 5, 35, (2, 1, 0), h=7, with_ln=False)
    assert all(c.bias is not None for c in ct.embd) and not any(k.startswith("embd_norm") for k in ct.state_dict())


def test_default_model_has_no_embedding_key_and_default_keys_change_nothing():
    a, b = tiny_cfg(8, (64, 96)), tiny_cfg(8, (64, 96))
    b.MODEL.EMBD_LAYERS, b.MODEL.FLOW_EMBD_LAYERS, b.MODEL.EMBD_KS, b.MODEL.EMBD_WITH_LN = 0, 0, 3, True
    ma, mb = OTPose(a), OTPose(b)
    assert not any(R.is_embd_key(k) for k in ma.state_dict())
    assert list(ma.state_dict()) == list(mb.state_dict())
    assert ma.scale_arch == (0, 6, 2) and ma.flow_scale_arch == (0, 6, 0)


def _embd_cfg(layers=1, flow=0, ks=3, ln=True):
    cfg = tiny_cfg(8, (64, 96))
    cfg.MODEL.EMBD_LAYERS, cfg.MODEL.FLOW_EMBD_LAYERS, cfg.MODEL.EMBD_KS, cfg.MODEL.EMBD_WITH_LN = layers, flow, ks, ln
    return cfg


def test_cfg_keys_build_the_embedding_layers():
    m = OTPose(_embd_cfg(2, 1, 5, False))
    for e in (m.temporal_encoder1, m.temporal_encoder2):
        assert [tuple(c.weight.shape) for c in e.embd] == [(136, 136, 5, 5)] * 2 and e.arch == (2, 6, 2)
        assert all(c.bias is not None for c in e.embd)
    assert [tuple(c.weight.shape) for c in m.flow_encoder.embd] == [(17, 17, 5, 5)] and m.flow_encoder.arch == (1, 6, 0)
    m = OTPose(_embd_cfg(1))
    assert len(m.flow_encoder.embd) == 0 and "temporal_encoder1.embd_norm.0.weight" in m.state_dict()
    # OTPose.init_weights treats them like every other Conv2d: N(0, 1e-3) weights
    w = m.temporal_encoder2.embd[0].weight.detach()
    assert 0.5e-3 < float(w.std()) < 2e-3


@pytest.mark.parametrize("kw", [dict(ks=2), dict(ks=7), dict(ks=3.0), dict(layers=-1), dict(flow=-2), dict(layers=1.5),
                                dict(ln="yes"), dict(layers=0, ks=4)])
def test_cfg_validation(kw):
    with pytest.raises(ValueError):
        OTPose(_embd_cfg(**kw))


def test_constructor_validation():
    with pytest.raises(ValueError, match="n_in"):
        M.ConvTransformer(24, 40, 2, 3, 35, (0, 1, 0), h=7)                 # nothing maps 24 -> 40
    with pytest.raises(ValueError, match="kernel size"):
        M.ConvTransformer(24, 40, 2, 2, 35, (1, 1, 0), h=7)
    with pytest.raises(ValueError):
        M.ConvTransformer(24, 320, 2, 3, 35, (1, 1, 0), h=7)
    with pytest.raises(ValueError):
        M.ConvTransformer(24, 40, 2, 3, 35, (-1, 1, 0), h=7)
    M.ConvTransformer(40, 40, 2, 4, 35, (0, 1, 0), h=7)                     # the kernel size is unused without a layer


def test_make_optimizer_groups_the_embedding_parameters():
    cfg = _embd_cfg(1, 1, 3, True)
    cfg.TRAIN.WD = 0.01
    m = OTPose(cfg)
    names = {id(p): n for n, p in m.named_parameters()}
    groups = [{names[id(p)] for p in pg["params"]} for pg in optim.make_optimizer(m, cfg).param_groups]
    wd = [pg["weight_decay"] for pg in optim.make_optimizer(m, cfg).param_groups]
    new = {n for n in names.values() if R.is_embd_key(n)}
    assert len(new) == 9                                                     # 3 encoders x (conv weight, norm weight, norm bias)
    for n in new:
        holders = [i for i, gset in enumerate(groups) if n in gset]
        assert len(holders) == 1
        assert (wd[holders[0]] == 0.01) == (".embd." in n and n.endswith("weight")), n
    assert set().union(*groups) == set(names.values()) and sum(len(gset) for gset in groups) == len(names)
    cfg = _embd_cfg(1, 0, 3, False)
    cfg.TRAIN.WD = 0.01
    m = OTPose(cfg)
    names = {id(p): n for n, p in m.named_parameters()}
    pgs = optim.make_optimizer(m, cfg).param_groups
    where = {names[id(p)]: pg["weight_decay"] for pg in pgs for p in pg["params"]}
    assert where["temporal_encoder1.embd.0.bias"] == 0.0 and where["temporal_encoder1.embd.0.weight"] == 0.01


def test_supported_predicate_and_argument_errors():
    L = hip.lib()
    for ok in [(16, 136, 96, 72, 136, 3), (16, 17, 96, 72, 17, 3), (1, 1, 1, 1, 1, 1), (2, 256, 3, 70, 256, 5), (1, 24, 7, 5, 40, 5)]:
        assert L.otp_conv_embd_supported(*ok) == 1, ok
    for no in [(1, 136, 12, 8, 136, 2), (1, 136, 12, 8, 136, 7), (1, 136, 12, 8, 257, 3), (1, 257, 12, 8, 136, 3),
               (0, 136, 12, 8, 136, 3), (1, 136, 0, 8, 136, 3), (1, 136, 12, 0, 136, 3), (1, 0, 12, 8, 136, 3),
               (1, 136, 1 << 16, 1 << 15, 136, 3)]:
        assert L.otp_conv_embd_supported(*no) == 0, no
    bad = hip.CONSTANTS["OTP_ERR_BAD_ARG"]
    p = ctypes.c_void_p(256)            # never dereferenced: every call below returns before a launch
    assert L.otp_conv_embd_weight_bytes(136, 136, 3) == 9 * 136 * 192 * 4 and L.otp_conv_embd_weight_bytes(17, 17, 5) == 25 * 20 * 32 * 4
    assert L.otp_conv_embd_weight_bytes(136, 136, 2) == 0 and L.otp_conv_embd_weight_bytes(136, 257, 3) == 0
    assert L.otp_conv_embd_pack_weight(p, p, 136, 136, 2, None) == bad
    assert L.otp_conv_embd_pack_weight(None, p, 136, 136, 3, None) == bad
    args = lambda **k: tuple({**dict(x=p, w=p, bias=None, g=p, b=p, pe=None, out=p, z=None, B=1, Cin=136, H=12, W=8, Cout=136,   # noqa: E731
                                     ks=3, eps=1e-5, st=None), **k}.values())
    assert L.otp_conv_embd(*args(ks=2)) == bad
    assert L.otp_conv_embd(*args(Cout=257)) == bad
    assert L.otp_conv_embd(*args(x=None)) == bad
    assert L.otp_conv_embd(*args(out=None)) == bad
    assert L.otp_conv_embd(*args(b=None)) == bad                            # gamma without beta
    assert L.otp_conv_embd(*args(B=0)) == bad
    n = L.otp_conv_embd_backward_pre_workspace(2, 136, 96)
    assert n == 2 * 2 * 2 * 136 * 4 and L.otp_conv_embd_backward_pre_workspace(2, 257, 96) == 0
    bw = lambda **k: tuple({**dict(z=p, bias=None, g=p, b=p, gy=p, gz=p, gg=p, gb=p, ws=p, n=n, B=2, C=136, T=96, eps=1e-5,     # noqa: E731
                                   st=None), **k}.values())
    assert L.otp_conv_embd_backward_pre(*bw(z=None)) == bad
    assert L.otp_conv_embd_backward_pre(*bw(C=257)) == bad
    assert L.otp_conv_embd_backward_pre(*bw(g=None)) == bad
    assert L.otp_conv_embd_backward_pre(*bw(ws=None)) == bad
    assert L.otp_conv_embd_backward_pre(*bw(g=None, b=None)) == bad        # no norm: there is no grad_gamma to write
    assert L.otp_conv_embd_backward_pre(*bw(n=n - 4)) == hip.CONSTANTS["OTP_ERR_WORKSPACE"]


def test_ops_raise_value_error_before_any_launch():
    from otpose_amd import ops, train_ops
    x, w = torch.zeros(1, 24, 7, 5), torch.zeros(40, 24, 3, 3)
    ops.conv_embd_params(x.shape, w, None, torch.ones(1, 40, 1), torch.zeros(1, 40, 1), torch.zeros(40, 35), "cpu")
    for bad in [dict(w=torch.zeros(40, 24, 2, 2)), dict(w=torch.zeros(257, 24, 3, 3)), dict(w=torch.zeros(40, 25, 3, 3)),
                dict(w=torch.zeros(40, 24, 3, 5)), dict(bias=torch.zeros(39)), dict(g=torch.ones(1, 41, 1)), dict(b=None),
                dict(pe=torch.zeros(40, 36)), dict(x=torch.zeros(1, 24, 35))]:
        a = {**dict(x=x, w=w, bias=None, g=torch.ones(1, 40, 1), b=torch.zeros(1, 40, 1), pe=None), **bad}
        with pytest.raises(ValueError):
            ops.conv_embd_params(a["x"].shape, a["w"], a["bias"], a["g"], a["b"], a["pe"], "cpu")
    with pytest.raises(ValueError, match="training"):
        train_ops.check_conv_embd_train((40, 24, 5, 5))
    train_ops.check_conv_embd_train((40, 24, 3, 3))


def test_restatement_is_the_layer_by_definition():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 3, 4, 5, generator=g, dtype=torch.float64)
    w = torch.randn(2, 3, 3, 3, generator=g, dtype=torch.float64)
    gamma, beta = torch.tensor([1.5, -0.5], dtype=torch.float64), torch.tensor([0.1, 0.2], dtype=torch.float64)
    pe = torch.randn(2, 20, generator=g, dtype=torch.float64)
    y = R.conv_embd(x, w, None, gamma, beta, pe)
    xp = torch.zeros(3, 6, 7, dtype=torch.float64)
    xp[:, 1:5, 1:6] = x[0]
    for yy in range(4):
        for xx in range(5):
            z = torch.stack([(w[o] * xp[:, yy:yy + 3, xx:xx + 3]).sum() for o in range(2)])
            mu = z.mean()
            v = (z - mu) / torch.sqrt(((z - mu) ** 2).mean() + 1e-5) * gamma + beta
            assert torch.allclose(y[0, :, yy * 5 + xx], v.clamp_min(0) + pe[:, yy * 5 + xx], atol=1e-12)
