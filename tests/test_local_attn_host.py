"""Local-window attention on the CPU: tests/local_attn_ref.py against the reference's own classes (tests/golden/local_attn.npz,
the restatement-equals-reference step of SURVEY.md section 7), the parameter containers' key sets, the optimizer grouping of
``rel_pe``, constructor / cfg validation, and the argument checks of the C entry points (which return before touching a GPU)."""
import ctypes

import pytest
import torch

from otpose_amd import OTPose, hip, tiny_cfg
from otpose_amd import modules as M
from otpose_amd import optim
from tests import local_attn_ref as R

TOL = 1e-5      # restatement vs reference, relative to max(1, max|ref|); observed 2e-7


def _rel(g, tag):
    pre = tag + "_rel/"
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


def _sd(module, seed, g, tag):
    R.fill_windowed_(module, seed, _rel(g, tag))
    return {k: v.detach() for k, v in module.state_dict().items()}


def _close(got, ref, tol=TOL):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = float((got - ref).abs().max())
    assert err <= tol * max(1.0, float(ref.abs().max())), err


@pytest.mark.parametrize("tag,c,nh,win,stride", [("lmhca_136_s1", 136, 2, 9, 1), ("lmhca_136_s2", 136, 2, 9, 2),
                                                 ("lmhca_17_s1", 17, 1, 5, 1)])
def test_restatement_matches_reference_local_mhca(golden, tag, c, nh, win, stride):
    g = golden("local_attn")
    sd = _sd(M.LocalMaskedMHCA(c, nh, win, stride, stride, proj_pdrop=0.1, use_rel_pe=True), 11, g, tag)
    _close(R.local_mhca({"a." + k: v for k, v in sd.items()}, "a", g[tag + "_x"], nh, stride, win), g[tag + "_y"])


@pytest.mark.parametrize("tag,c,nh,stride", [("ltblock_136_s1", 136, 2, 1), ("ltblock_136_s2", 136, 2, 2),
                                             ("ltblock_17_s1", 17, 1, 1)])
def test_restatement_matches_reference_transformer_block(golden, tag, c, nh, stride):
    g = golden("local_attn")
    blk = M.TransformerBlock(c, nh, (stride, stride), 0.1, 0.1, 0.1, mha_win_size=9, use_rel_pe=True)
    sd = _sd(blk, 12, g, tag)
    _close(R.transformer_block({"b." + k: v for k, v in sd.items()}, "b", g[tag + "_x"], nh, stride, 9), g[tag + "_y"])


def test_restatement_matches_reference_conv_transformer(golden):
    g = golden("local_attn")
    ct = M.ConvTransformer(136, 136, 2, 3, 96, (0, 2, 2), h=12, proj_pdrop=0.1, path_pdrop=0.1, mha_win_size=[9, 9, 5],
                           use_rel_pe=True)
    assert [type(b.attn).__name__ for b in list(ct.stem) + list(ct.branch)] == ["LocalMaskedMHCA"] * 4
    assert [b.attn.window_size for b in list(ct.stem) + list(ct.branch)] == [9, 9, 9, 5]
    sd = _sd(ct, 14, g, "lct_136")
    x = g["lct_136_x"]
    for i, y in enumerate(R.conv_transformer({"c." + k: v for k, v in sd.items()}, "c", x, 2, (0, 2, 2), [9, 9, 5])):
        _close(y, g[f"lct_136_y{i}"].reshape(y.shape))


def test_windowed_block_key_set_is_the_reference_one_and_defaults_are_unchanged():
    import numpy as np
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "local_attn.npz"))
    want = [str(k) for k in z["ltblock_keys"]]
    blk = M.TransformerBlock(136, 2, (1, 1), 0.1, 0.1, 0.1, mha_win_size=9, use_rel_pe=True)
    assert sorted(blk.state_dict()) == want
    assert tuple(blk.attn.rel_pe.shape) == (1, 1, 2, 9)
    std = (2.0 / 136) ** 0.5
    assert 0 < float(blk.attn.rel_pe.detach().abs().max()) <= 2 * std
    plain = M.TransformerBlock(136, 2, (1, 1), 0.1, 0.1, 0.1)
    assert type(plain.attn) is M.MaskedMHCA
    assert sorted(plain.state_dict()) == [k for k in want if k != "attn.rel_pe"]
    no_rel = M.TransformerBlock(136, 2, (1, 1), mha_win_size=9)
    assert type(no_rel.attn) is M.LocalMaskedMHCA and "attn.rel_pe" not in no_rel.state_dict()
    # a model built without the keys and one with them at their defaults own the same keys
    a, b = tiny_cfg(8, (64, 96)), tiny_cfg(8, (64, 96))
    b.MODEL.MHA_WIN_SIZE, b.MODEL.USE_REL_PE, b.MODEL.FLOW_MHA_WIN_SIZE = -1, False, -1
    assert list(OTPose(a).state_dict()) == list(OTPose(b).state_dict())


def _windowed_cfg(win=9, rel=True, flow=-1, size=(64, 96)):
    cfg = tiny_cfg(8, size)
    cfg.MODEL.MHA_WIN_SIZE, cfg.MODEL.USE_REL_PE, cfg.MODEL.FLOW_MHA_WIN_SIZE = win, rel, flow
    return cfg


def test_cfg_keys_build_windowed_encoders():
    m = OTPose(_windowed_cfg(9, True, 5))
    rel = [k for k in m.state_dict() if k.endswith("rel_pe")]
    assert len(rel) == 16 and all(k.startswith("temporal_encoder") for k in rel)       # 2 encoders x (6 stem + 2 branch)
    assert all(type(b.attn) is M.LocalMaskedMHCA and b.attn.window_size == 5 and not b.attn.use_rel_pe
               for b in m.flow_encoder.stem)
    m = OTPose(_windowed_cfg([9, -1, 5], False))
    e = m.temporal_encoder1
    assert type(e.stem[0].attn) is M.LocalMaskedMHCA and type(e.branch[0].attn) is M.MaskedMHCA
    assert e.branch[1].attn.window_size == 5


def test_make_optimizer_puts_rel_pe_into_the_no_decay_group():
    cfg = _windowed_cfg()
    cfg.TRAIN.WD = 0.01
    m = OTPose(cfg)
    opt = optim.make_optimizer(m, cfg)
    names = {id(p): n for n, p in m.named_parameters()}
    groups = [{names[id(p)] for p in pg["params"]} for pg in opt.param_groups]
    rel = {n for n in names.values() if n.endswith("rel_pe")}
    assert len(rel) == 16
    holders = [i for i, gset in enumerate(groups) if rel & gset]
    assert len(holders) == 1 and rel <= groups[holders[0]] and opt.param_groups[holders[0]]["weight_decay"] == 0.0
    assert set().union(*groups) == set(names.values()) and sum(len(gset) for gset in groups) == len(names)


@pytest.mark.parametrize("win", [8, 3, 35, 1.5])
def test_constructor_rejects_unsupported_windows(win):
    with pytest.raises(ValueError):
        M.LocalMaskedMHCA(136, 2, win)
    with pytest.raises(ValueError):
        M.TransformerBlock(136, 2, (1, 1), mha_win_size=win)
    with pytest.raises(ValueError):
        OTPose(_windowed_cfg(win))


def test_cfg_validation_names_the_level_that_does_not_divide():
    # heat-map 16 x 24: T = 384 / 192 / 96; window 17 needs multiples of 16: fine; 33 needs 32: fine; 25 needs 24: 384 ok, 192 ok, 96 ok
    OTPose(_windowed_cfg(17))
    # heat-map 24 x 40 (image 96 x 160): T = 960 / 480 / 240; window 33 -> 32 divides 960 and 480 but not 240
    with pytest.raises(ValueError, match=r"MHA_WIN_SIZE\[2\].*level 2"):
        OTPose(_windowed_cfg(33, size=(96, 160)))
    OTPose(_windowed_cfg([33, 33, 9], size=(96, 160)))
    with pytest.raises(ValueError, match="FLOW_MHA_WIN_SIZE"):
        OTPose(_windowed_cfg(-1, False, flow=11))                                     # 384 % 10
    with pytest.raises(ValueError, match="entries"):
        OTPose(_windowed_cfg([9, 9]))


def test_supported_predicate_and_argument_errors():
    L = hip.lib()
    assert L.otp_local_attn_supported(68, 6912, 9) == 1 and L.otp_local_attn_supported(17, 6912, 19) == 1
    assert L.otp_local_attn_supported(102, 1056, 33) == 1 and L.otp_local_attn_supported(17, 4, 5) == 1
    for hs, t, win in [(68, 6912, 8), (68, 6912, 3), (68, 6912, 35), (68, 6910, 9), (0, 8, 9), (68, 0, 9), (68, 8, -9)]:
        assert L.otp_local_attn_supported(hs, t, win) == 0, (hs, t, win)
    bad = hip.CONSTANTS["OTP_ERR_BAD_ARG"]
    p = ctypes.c_void_p(256)            # never dereferenced: every call below returns before a launch
    assert L.otp_local_attn(None, p, p, None, p, None, 1, 136, 96, 2, 9, 0.1, None) == bad
    assert L.otp_local_attn(p, p, p, None, None, None, 1, 136, 96, 2, 9, 0.1, None) == bad
    assert L.otp_local_attn(p, p, p, None, p, None, 1, 136, 96, 2, 8, 0.1, None) == bad       # even window
    assert L.otp_local_attn(p, p, p, None, p, None, 1, 136, 100, 2, 9, 0.1, None) == bad      # T % 8
    assert L.otp_local_attn(p, p, p, None, p, None, 1, 135, 96, 2, 9, 0.1, None) == bad       # C % n_head
    assert L.otp_local_attn(p, p, p, None, p, None, 0, 136, 96, 2, 9, 0.1, None) == bad
    n = L.otp_local_attn_backward_workspace(2, 136, 96, 2, 9)
    assert n == (4 * 96 + 4 * 1) * 9 * 4 and L.otp_local_attn_backward_workspace(16, 136, 6912, 2, 9) > 0
    assert L.otp_local_attn_backward_workspace(2, 136, 96, 2, 8) == 0
    assert L.otp_local_attn_backward(p, p, p, None, p, p, p, p, None, p, n, 2, 136, 96, 2, 9, 0.1, None) == bad
    assert L.otp_local_attn_backward(p, p, p, p, p, p, p, p, None, None, n, 2, 136, 96, 2, 9, 0.1, None) == bad
    assert L.otp_local_attn_backward(p, p, p, p, p, p, p, p, None, p, n, 2, 136, 96, 2, 7 + 1, 0.1, None) == bad
    assert L.otp_local_attn_backward(p, p, p, p, p, p, p, p, None, p, n - 4, 2, 136, 96, 2, 9, 0.1, None) == \
        hip.CONSTANTS["OTP_ERR_WORKSPACE"]


def test_ops_raise_value_error_before_any_launch():
    from otpose_amd import ops
    with pytest.raises(ValueError):
        ops.check_local_attn(136, 96, 2, 8)
    with pytest.raises(ValueError):
        ops.check_local_attn(136, 100, 2, 9)
    with pytest.raises(ValueError):
        ops.check_local_attn(135, 96, 2, 9)
    ops.check_local_attn(136, 96, 2, 9)


def test_restatement_is_a_softmax_over_the_positions_inside_the_sequence():
    q, k, v = (torch.randn(1, 6, 8, generator=torch.Generator().manual_seed(s), dtype=torch.float64) for s in (1, 2, 3))
    p = R.local_attn_probs(q, k, 2, 5, 0.3)
    assert torch.allclose(p.sum(-1), torch.ones(1, 2, 8, dtype=torch.float64))
    assert float(p[0, :, 0, :2].abs().max()) == 0 and float(p[0, :, 7, 3:].abs().max()) == 0 and float(p[0, :, 1, 0].abs().max()) == 0
    # token by token against the definition
    out = R.local_attn(q, k, v, 2, 5, 0.3)
    for h in range(2):
        for t in range(8):
            js = [j for j in range(5) if 0 <= t + j - 2 < 8]
            s = torch.stack([0.3 * (q[0, 3 * h:3 * h + 3, t] * k[0, 3 * h:3 * h + 3, t + j - 2]).sum() for j in js])
            pr = torch.softmax(s, 0)
            o = sum(pr[i] * v[0, 3 * h:3 * h + 3, t + j - 2] for i, j in enumerate(js))
            assert torch.allclose(out[0, 3 * h:3 * h + 3, t], o, atol=1e-12)


def test_windowed_state_dict_round_trips_by_name(tmp_path):
    from otpose_amd import checkpoints
    a, b = OTPose(_windowed_cfg()), OTPose(_windowed_cfg())
    with torch.no_grad():
        for k, v in a.state_dict().items():
            if k.endswith("rel_pe"):
                v.normal_()
    path = tmp_path / "w.pth"
    torch.save({"state_dict": a.state_dict()}, path)
    sd = torch.load(path, map_location="cpu")["state_dict"]
    assert b.load_state_dict(sd, strict=True).missing_keys == []
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    with pytest.raises(RuntimeError, match="rel_pe"):
        OTPose(tiny_cfg(8, (64, 96))).load_state_dict(sd, strict=True)          # a model without windows has nowhere to put it
    assert checkpoints is not None
