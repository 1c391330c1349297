"""RSN_ATTENTION / RSN_WEIGHT_VECTOR without a GPU: the restatement of tests/prm_ref.py against the reference's own outputs
(tests/golden/prm.npz), the containers' key sets, the ``MODEL.PRM`` extension key, the optimizer groups, and the ReLU-kink accounting
of the gradient tests in tests/test_gpu_prm.py."""
import functools
import os

import numpy as np
import pytest
import torch

from otpose_amd import OTPose, tiny_cfg
from otpose_amd import modules as M
from otpose_amd.optim import make_optimizer, reference_param_groups
from tests import prm_ref as R
from tests.conftest import seeded

D = torch.float64
PRM_BOTH = ("def_fuse", "offset_mask_combine_conv")
# tag -> (class, constructor arguments, input shape, weight seed, input seed): the cases of tests/golden/make_golden_prm.py
CASES = {
    "att_17": ("RSN_ATTENTION", (17,), (2, 17, 5, 7), 31, 41),
    "att_32": ("RSN_ATTENTION", (32,), (1, 32, 13, 19), 32, 42),
    "vec_17_20": ("RSN_WEIGHT_VECTOR", (17, 20), (2, 17, 6, 9), 33, 43),
}
# the training-mode cases of tests/test_gpu_prm.py: (N, C, H, W); N = 4 and 5 (with N = 2 the gate BatchNorm outputs are +-1 and
# their gradient degenerate); 5 x 7 keeps every 9x9 tap on the border, 13 x 19 has interior pixels
TRAIN_SHAPES = [(4, 17, 5, 7), (5, 20, 13, 19)]


def build_case(tag):
    cls, args, _, wseed, _ = CASES[tag]
    return R.fill_prm_(getattr(M, cls)(*args), wseed).eval()


@pytest.mark.parametrize("tag", sorted(CASES))
def test_restatement_matches_reference_outputs(golden, tag):
    g = golden("prm")
    sd = {k: v.detach() for k, v in build_case(tag).state_dict().items()}
    fn = R.rsn_attention if CASES[tag][0] == "RSN_ATTENTION" else R.rsn_weight_vector
    for dtype in (torch.float32, D):
        y = fn({k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}, "", g[tag + "_x"].to(dtype))
        assert y.shape == g[tag + "_y"].shape
        assert float((y - g[tag + "_y"]).abs().max()) <= 1e-5


@pytest.mark.parametrize("tag", ["att_17", "att_32"])
def test_folded_operator_restatement_equals_the_module_restatement(golden, tag):
    g = golden("prm")
    sd = {k: v.detach().double() for k, v in build_case(tag).state_dict().items()}
    x = g[tag + "_x"].double()
    f = R.cbr(sd, "conv_bn_relu_prm_1", x)
    gate = R.prm_gate(f, *R.fold(sd, "conv_bn_relu_prm_2_1"), *R.fold(sd, "conv_bn_relu_prm_2_2"))
    y = R.prm_apply(f, gate, *R.fold(sd, "conv_bn_relu_prm_3_1"), *R.fold(sd, "conv_bn_relu_prm_3_2"))
    assert float((y - R.rsn_attention(sd, "", x)).abs().max()) <= 1e-12


def test_weight_vector_folded_restatement_uses_the_residual(golden):
    g = golden("prm")
    sd = {k: v.detach().double() for k, v in build_case("vec_17_20").state_dict().items()}
    x = g["vec_17_20_x"].double()
    f = R.cbr(sd, "conv_bn_relu_1", x)
    folded = (*R.fold(sd, "conv_bn_relu_2"), *R.fold(sd, "conv_bn_relu_3"))
    ref = R.rsn_weight_vector(sd, "", x)
    assert float((R.prm_gate(f, *folded, residual=True) - ref).abs().max()) <= 1e-12
    assert float((R.prm_gate(f, *folded, residual=False) - ref).abs().max()) > 1e-4


@pytest.mark.parametrize("tag", sorted(CASES))
def test_container_keys_and_shapes_equal_the_reference_classes(tag):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "prm.npz"))      # (the fixture drops the string arrays)
    sd = build_case(tag).state_dict()
    assert sorted(sd) == [str(k) for k in z[tag + "_keys"]]
    assert [",".join(str(d) for d in sd[k].shape) for k in sorted(sd)] == [str(s) for s in z[tag + "_shapes"]]


def test_conv_bn_relu_groups_default_leaves_the_key_set_untouched():
    a, b = M.conv_bn_relu(8, 8, 3, 1, 1), M.conv_bn_relu(8, 8, 3, 1, 1, groups=1, efficient=True)
    assert {k: v.shape for k, v in a.state_dict().items()} == {k: v.shape for k, v in b.state_dict().items()}
    assert tuple(M.conv_bn_relu(8, 8, 9, 1, 4, groups=8).conv.weight.shape) == (8, 1, 9, 9)
    assert isinstance(M.RSN_ATTENTION(8, efficient=True), M.RSN_ATTENTION)


def _keys(cfg):
    return {k: tuple(v.shape) for k, v in OTPose(cfg).state_dict().items()}


def test_empty_prm_key_gives_the_default_key_set():
    cfg = tiny_cfg(8, (64, 96))
    cfg.MODEL.PRM = ()
    base = _keys(tiny_cfg(8, (64, 96)))
    assert _keys(cfg) == base
    cfg.MODEL.PRM = PRM_BOTH
    both = _keys(cfg)
    extra = set(both) - set(base)
    assert set(base) <= set(both) and extra and all(k.startswith(("def_fuse_prm.", "offset_mask_combine_prm.")) for k in extra)
    assert both["def_fuse_prm.conv_bn_relu_prm_3_2.conv.weight"] == (cfg.MODEL.NUM_JOINTS, 1, 9, 9)
    assert both["offset_mask_combine_prm.conv_bn_relu_prm_1.conv.weight"][:2] == (cfg.MODEL.DEFORMABLE_CONV_CH,) * 2
    cfg.MODEL.PRM = ["def_fuse"]
    assert not any(k.startswith("offset_mask_combine_prm.") for k in _keys(cfg))


@pytest.mark.parametrize("bad", ["def_fuse", ("final_layer1",), ("def_fuse", "def_fuse"), (1,), None, 3])
def test_malformed_prm_key_raises(bad):
    cfg = tiny_cfg(8, (64, 96))
    cfg.MODEL.PRM = bad
    with pytest.raises(ValueError, match="MODEL.PRM"):
        OTPose(cfg)


def test_more_than_64_channels_raise():
    for make in (lambda: M.RSN_ATTENTION(65), lambda: M.RSN_WEIGHT_VECTOR(17, 65), lambda: M.RSN_ATTENTION(0)):
        with pytest.raises(ValueError):
            make()
    M.RSN_ATTENTION(64)
    cfg = tiny_cfg(8, (64, 96))
    cfg.MODEL.PRM, cfg.MODEL.DEFORMABLE_CONV_CH = PRM_BOTH, 96
    with pytest.raises(ValueError):
        OTPose(cfg)


def test_make_optimizer_covers_every_parameter_with_the_key_on():
    cfg = tiny_cfg(8, (64, 96))
    cfg.MODEL.PRM = PRM_BOTH
    m = OTPose(cfg)
    groups = reference_param_groups(m, cfg)              # (asserts that every parameter is in exactly one group)
    names = {id(p): n for n, p in m.named_parameters()}
    where = {names[id(p)]: i for i, g in enumerate(groups) for p in g["params"]}
    assert len(where) == len(names)
    for prm, chain in (("def_fuse_prm", "def_fuse"), ("offset_mask_combine_prm", "offset_mask_combine_conv")):
        for layer in R.ATT_LAYERS:
            for leaf, twin in (("conv.weight", "conv.weight"), ("conv.bias", "conv.bias"), ("bn.weight", "bn.weight"),
                               ("bn.bias", "bn.bias")):
                assert where[f"{prm}.{layer}.{leaf}"] == where[f"{chain}.layers.0.conv_bn_relu1.{twin}"], (prm, layer, leaf)
    opt = make_optimizer(m, cfg, fused=False)
    assert sum(len(g["params"]) for g in opt.param_groups) == len(names)


# ---- the training cases of the GPU tests and their ReLU kinks ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def train_case(shape):
    """(state dict (fp32), x, cotangent) of the whole-module training test at ``shape``.  The input seeds are ones at which no ReLU
    pre-activation of the float64 run lies within KINK_DELTA of zero (the smallest: 6.0e-5 and 1.3e-5), so nothing is left out."""
    n, c, h, w = shape
    mod = R.fill_prm_(M.RSN_ATTENTION(c), 50 + n)
    sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    return sd, seeded(shape, 61 + n), seeded(shape, 70 + n)


@functools.lru_cache(maxsize=None)
def train_reference(shape, dtype):
    """Output, gradients (x, then every parameter by name), batch statistics and ReLU pre-activations of the restatement in
    batch-statistics mode."""
    sd, x, go = train_case(shape)
    names = [k for k, v in sd.items() if v.is_floating_point() and "running_" not in k]
    leaves = {k: sd[k].detach().clone().to(dtype).requires_grad_() for k in names}
    full = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
    full.update(leaves)
    xl = x.detach().clone().to(dtype).requires_grad_()
    pre, stats = {}, {}
    out = R.rsn_attention(full, "", xl, train=True, pre=pre, stats=stats)
    grads = torch.autograd.grad(out, [xl] + [leaves[k] for k in names], go.to(dtype))
    return out.detach(), grads[0], dict(zip(names, grads[1:])), stats, pre


@pytest.mark.parametrize("shape", TRAIN_SHAPES)
def test_relu_kinks_of_the_training_cases_stay_inside_the_cap(shape):
    """An element may be left out of a gradient comparison only if a ReLU pre-activation feeding it lies within KINK_DELTA of zero
    in the float64 run: at most KINK_CAP of any tensor, and no gate-vector pre-activation at all."""
    *_, pre = train_reference(shape, D)
    report = R.kink_report(pre)
    assert len(report) == 5 and sum(vec for _, vec in report.values()) == 2
    for layer, (share, is_vector) in report.items():
        assert share <= R.KINK_CAP, (layer, share)
        if is_vector:
            assert share == 0.0, (layer, share)
    assert float(R.kink_pixels(pre, shape).double().mean()) <= R.KINK_CAP


def test_one_value_per_channel_is_refused_in_batch_statistics_mode():
    sd, x, _ = train_case(TRAIN_SHAPES[0])
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        R.rsn_attention(sd, "", x[:1], train=True)
    assert R.rsn_attention(sd, "", x[:1]).shape == x[:1].shape           # eval mode takes N = 1
