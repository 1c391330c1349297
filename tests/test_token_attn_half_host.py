"""Token attention with half products without a GPU: the four C symbols and their host side, the ``products`` argument of the
Python face, the ``MODEL.TOKEN_PRODUCTS`` key, and the rounded restatement (tests/token_attn_half_ref.py) against the exact one
with its rounding switched off."""
import ctypes

import pytest
import torch

from otpose_amd import hip
from otpose_amd import token_attn as TA
from tests import token_attn_half_ref as H
from tests import token_attn_ref as R

SYMBOLS = ("otp_token_attn_h1_supported", "otp_token_attn_forward_h1", "otp_token_attn_backward_h1", "otp_token_attn_h1_workspace")


def test_header_declares_and_library_exports_the_symbols():
    cdll = ctypes.CDLL(hip.LIB_PATH)
    for name in SYMBOLS:
        assert name in hip.SIGNATURES, name
        assert getattr(cdll, name) is not None, name
    fwd, bwd = hip.SIGNATURES["otp_token_attn_forward_h1"][1], hip.SIGNATURES["otp_token_attn_backward_h1"][1]
    # the fp32 entry points' lists, then (p, seed) of the dropout, the range-guard word, and the stream last as everywhere
    tail = [ctypes.c_float, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p]
    assert fwd == hip.SIGNATURES["otp_token_attn_forward"][1][:-1] + tail
    assert bwd == hip.SIGNATURES["otp_token_attn_backward"][1][:-1] + tail


def test_supported_equals_the_fp32_query():
    L = hip.lib()
    table = [(136, 1, 200), (137, 1, 200), (272, 2, 6912), (274, 2, 6912), (136, 3, 200), (136, 2, 0), (5, 1, 1), (17, 1, 35),
             (0, 1, 5), (16, 0, 5)]
    assert [L.otp_token_attn_h1_supported(*a) for a in table] == [1, 0, 1, 0, 0, 0, 1, 1, 0, 0]
    for a in table + [(-3, 1, 4), (16, -1, 4), (16, 2, -1), (16, 16, 1), (2176, 16, 3), (2192, 16, 3)]:
        assert L.otp_token_attn_h1_supported(*a) == L.otp_token_attn_supported(*a), a


@pytest.mark.parametrize("b,nh,t,hd", [(16, 2, 6912, 68), (1, 1, 1, 1), (2, 8, 333, 17)])
def test_workspace_does_not_grow_with_t_squared(b, nh, t, hd):
    n = hip.lib().otp_token_attn_h1_workspace(b, nh, t, hd)
    assert 0 < n <= 16 * b * nh * t + 4096


def test_entry_points_return_bad_arg_on_null_pointers():
    L = hip.lib()
    assert L.otp_token_attn_forward_h1(None, None, None, None, None, None, 1, 16, 2, 8, 1.0, 0.0, 0, None, None) == -1
    assert L.otp_token_attn_backward_h1(None, None, None, None, None, None, None, None, None, None, None, 1, 16, 2, 8, 1.0, 0.0, 0,
                                        None, None) == -1


def test_products_argument_is_validated_before_the_device_is_asked():
    q = torch.zeros(2, 34, 16)
    for bad in ("bf16", "fp16", "", None, 16):
        with pytest.raises(ValueError, match="products"):
            TA.token_attn(q, q, q, 2, 1.0, products=bad)
    with pytest.raises(ValueError, match="heads"):
        TA.token_attn(q, q, q, 3, 1.0, products="half")
    with pytest.raises(NotImplementedError):
        TA.token_attn(q, q, q, 2, 1.0, products="half")             # well-formed, but on the CPU
    with pytest.raises(NotImplementedError):
        TA.token_attn(q, q, q, 2, 1.0, products="f32")


def test_layer_products_attribute():
    from otpose_amd import modules as M
    layer = M.TransformerEncoderLayer(136, 2, 272)
    keys = sorted(layer.state_dict())
    assert layer.products == "f32"
    assert layer.set_products("half") is layer and layer.products == "half"
    assert sorted(layer.state_dict()) == keys
    for bad in ("bf16", None, 1):
        with pytest.raises(ValueError, match="products"):
            layer.set_products(bad)
    assert layer.products == "half"
    enc = M.TransformerEncoder(layer, 2)                            # the clones carry the mode of the layer they were copied from
    assert [l.products for l in enc.layers] == ["half", "half"]


# ---- MODEL.TOKEN_PRODUCTS -------------------------------------------------------------------------------------------------------------
def _keyed_cfg(**keys):
    from otpose_amd import tiny_cfg
    cfg = tiny_cfg(8, (64, 96))
    for k, v in keys.items():
        cfg.MODEL[k] = v
    return cfg


@pytest.mark.parametrize("value", ["bf16", "HALF", "", None, 16, True, ("half",)])
def test_bad_token_products_raise_naming_the_key(value):
    """Rejected also with no layer asked for, like the other TOKEN_* keys."""
    from otpose_amd import OTPose
    with pytest.raises(ValueError, match="MODEL.TOKEN_PRODUCTS"):
        OTPose(_keyed_cfg(TOKEN_PRODUCTS=value))


def test_token_products_reach_all_three_encoders_and_add_no_key():
    from otpose_amd import OTPose
    absent = OTPose(_keyed_cfg(TOKEN_LAYERS=2, FLOW_TOKEN_LAYERS=1))
    assert absent.token_keys["products"] == "f32"
    encoders = ("token_encoder1", "token_encoder2", "flow_token_encoder")
    assert {l.products for n in encoders for l in getattr(absent, n).layers} == {"f32"}
    for mode in ("f32", "half"):
        m = OTPose(_keyed_cfg(TOKEN_LAYERS=2, FLOW_TOKEN_LAYERS=1, TOKEN_PRODUCTS=mode))
        assert [l.products for n in encoders for l in getattr(m, n).layers] == [mode] * 5
        assert sorted(m.state_dict()) == sorted(absent.state_dict())
    plain = OTPose(_keyed_cfg())
    assert sorted(OTPose(_keyed_cfg(TOKEN_PRODUCTS="half")).state_dict()) == sorted(plain.state_dict())


# ---- the rounded restatement ----------------------------------------------------------------------------------------------------------
def _case(b, c, nh, t, seed, masked):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(b, c, t, generator=g, dtype=torch.float64) for _ in range(3))
    mask = None
    if masked:
        mask = torch.rand(b, t, generator=g) < 0.4
        mask[:, 0] = False
    return q, k, v, mask, torch.randn(b, c, t, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("b,c,nh,t,masked", [(2, 34, 2, 65, False), (2, 34, 2, 65, True), (1, 17, 1, 35, True), (1, 1, 1, 1, False)])
def test_restatement_without_rounding_is_the_exact_operator(b, c, nh, t, masked):
    q, k, v, mask, go = _case(b, c, nh, t, 5, masked)
    scale = (c // nh) ** -0.5
    ref, gref = R.autograd(lambda q_, k_, v_: R.token_attn(q_, k_, v_, nh, scale, mask), (q, k, v), go)
    got, ggot = R.autograd(lambda q_, k_, v_: H.token_attn(q_, k_, v_, nh, scale, mask, rounding=False), (q, k, v), go)
    assert float((got - ref).abs().max()) <= 1e-12
    for a, r in zip(ggot, gref):
        assert float((a - r).abs().max()) <= 1e-12


def test_rounding_moves_the_restatement_by_about_a_half_ulp_and_inside_the_bound():
    q, k, v, mask, go = _case(2, 34, 2, 65, 6, True)
    scale = 17 ** -0.5
    ref = R.token_attn(q, k, v, 2, scale, mask)
    got, grads = R.autograd(lambda q_, k_, v_: H.token_attn(q_, k_, v_, 2, scale, mask), (q, k, v), go)
    err = float((got - ref).abs().max())
    assert 1e-6 < err <= H.forward_bound(q, k, v, 2, scale, mask)
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    assert bool((grads[1][mask[:, None, :].expand_as(k)] == 0).all()) and bool((grads[2][mask[:, None, :].expand_as(v)] == 0).all())


def test_half_is_straight_through_and_exact_on_halves():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -12, 0.1, -65504.0], dtype=torch.float64, requires_grad=True)
    y = H.half(x)
    assert y.tolist() == [1.0, 1.0, float(torch.tensor(0.1).half()), -65504.0]
    y.sum().backward()
    assert x.grad.tolist() == [1.0] * 4
