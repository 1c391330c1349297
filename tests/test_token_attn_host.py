"""Token x token attention without a GPU: the plain-torch restatement of tests/token_attn_ref.py against the reference's own
TransformerEncoder outputs and attention maps (tests/golden/token_encoder.npz, 1e-5: the project's figure for fp32 restatements
against reference outputs), the sine tables against the reference's (1e-6), and the host side of the C entry points."""
import os

import numpy as np
import pytest
import torch

from otpose_amd import hip
from otpose_amd import token_attn as TA
from tests import token_attn_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_encoder.npz")
# tag -> (E, heads, FFN, activation, pre-norm, layers, final norm, pe_only_at_begin, maps): tests/golden/make_golden_token_encoder.py
CASES = {"a": (136, 2, 272, "gelu", False, 2, False, False, False), "b": (17, 1, 34, "relu", True, 2, True, False, True),
         "c": (136, 2, 272, "gelu", False, 2, False, True, False)}
WEIGHT_SEED = {"a": 10, "b": 40, "c": 10}
SINE = [(12, 9, 136), (5, 7, 8), (16, 12, 204)]


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _state(gold, tag):
    shapes = {k: tuple(int(d) for d in s.split(",")) for k, s in zip(gold[tag + "_keys"], gold[tag + "_shapes"])}
    return R.encoder_values(shapes, WEIGHT_SEED[tag])


@pytest.mark.parametrize("tag", sorted(CASES))
def test_restatement_matches_the_reference_encoder(gold, tag):
    e, nh, ffn, act, pre, layers, norm, pe_begin, maps = CASES[tag]
    sd = _state(gold, tag)
    assert ("norm.weight" in sd) == norm
    mask = torch.from_numpy(gold[tag + "_mask"]) if tag + "_mask" in gold else None
    if mask is not None:
        assert bool((~mask).any(dim=1).all()), "every sample of the fixture keeps a live key"
        assert sorted(int(c) for c in mask.sum(dim=1)) == [3, 11]
    y, amaps = R.encoder(sd, torch.from_numpy(gold[tag + "_x"]), layers, nh, act, pre, mask, torch.from_numpy(gold[tag + "_pos"]),
                         pe_begin)
    ref = torch.from_numpy(gold[tag + "_y"])
    err = float((y - ref).abs().max())
    print(f"TOKATTN|host {tag}|err {err:.3e}|max|ref| {float(ref.abs().max()):.3e}")
    assert err <= 1e-5 * max(1.0, float(ref.abs().max()))
    if maps:
        mref = torch.from_numpy(gold[tag + "_maps"])
        assert amaps.shape == mref.shape
        assert float((amaps - mref).abs().max()) <= 1e-5
        assert bool((amaps[:, mask[:, None, :].expand(amaps.shape[1:])] == 0).all())


def test_pos_only_at_begin_changes_the_output(gold):
    assert float(np.abs(gold["a_y"] - gold["c_y"]).max()) > 1e-3


@pytest.mark.parametrize("h,w,d", SINE)
def test_sine_tables_equal_the_reference(gold, h, w, d):
    ref = torch.from_numpy(gold[f"sine_{h}_{w}_{d}"])
    for name, got in (("package", TA.sine_position_embedding(h, w, d)), ("restatement", R.sine_table(h, w, d))):
        assert got.shape == ref.shape == (1, h * w, d), name
        assert float((got - ref).abs().max()) <= 1e-6, name
    assert np.array_equal(gold["a_pos"], gold["sine_12_9_136"].transpose(1, 0, 2))


@pytest.mark.parametrize("d", [17, 6, 0, -4, 8.0])
def test_sine_table_rejects_widths_that_are_no_multiple_of_four(d):
    with pytest.raises(ValueError):
        TA.sine_position_embedding(3, 3, d)


def test_recorded_key_lists_are_those_of_the_reference_classes(gold):
    layer = ["linear1.bias", "linear1.weight", "linear2.bias", "linear2.weight", "norm1.bias", "norm1.weight", "norm2.bias",
             "norm2.weight", "self_attn.in_proj_bias", "self_attn.in_proj_weight", "self_attn.out_proj.bias",
             "self_attn.out_proj.weight"]
    assert list(gold["a_layer_keys"]) == layer
    assert list(gold["a_keys"]) == sorted(f"layers.{i}.{k}" for i in range(2) for k in layer)
    assert list(gold["b_keys"]) == sorted([f"layers.{i}.{k}" for i in range(2) for k in layer] + ["norm.bias", "norm.weight"])
    shapes = dict(zip(gold["a_layer_keys"], gold["a_layer_shapes"]))
    assert shapes["self_attn.in_proj_weight"] == "408,136" and shapes["linear1.weight"] == "272,136"
    assert shapes["norm1.weight"] == "136" and shapes["self_attn.out_proj.weight"] == "136,136"


def _project_module(tag):
    from torch import nn
    from otpose_amd import modules as M
    e, nh, ffn, act, pre, layers, norm, pe_begin, maps = CASES[tag]
    layer = M.TransformerEncoderLayer(e, nh, ffn, activation=act, normalize_before=pre, return_atten_map=maps)
    return layer, M.TransformerEncoder(layer, layers, nn.LayerNorm(e) if norm else None, pe_begin, maps)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_project_modules_have_the_reference_key_sets_and_shapes(gold, tag):
    layer, enc = _project_module(tag)
    for mod, pre in ((layer, tag + "_layer"), (enc, tag)):
        sd = mod.state_dict()
        assert sorted(sd) == list(gold[pre + "_keys"])
        assert [",".join(str(d) for d in sd[k].shape) for k in sorted(sd)] == list(gold[pre + "_shapes"])
    assert {n for n, _ in enc.named_parameters()} == set(enc.state_dict())          # no buffers, every key trains


def test_project_encoder_initialises_like_the_reference():
    """xavier-uniform on every parameter of more than one dimension: bounded by sqrt(6 / (fan_in + fan_out)), and the clones
    are drawn separately; LayerNorm weights stay 1, the attention biases 0."""
    import math
    torch.manual_seed(3)
    _, enc = _project_module("a")
    for name, p in enc.state_dict().items():
        if p.dim() > 1:
            bound = math.sqrt(6.0 / (p.shape[0] + p.shape[1]))
            assert float(p.abs().max()) <= bound and float(p.abs().max()) > 0.9 * bound, name
        elif "norm" in name and name.endswith("weight"):
            assert bool((p == 1).all()), name
        elif "self_attn" in name:
            assert bool((p == 0).all()), name
    assert not torch.equal(enc.layers[0].linear1.weight, enc.layers[1].linear1.weight)


def test_project_module_deviations_raise():
    from otpose_amd import modules as M
    with pytest.raises(ValueError, match="activation"):
        M.TransformerEncoderLayer(136, 2, 272, activation="glu")
    with pytest.raises(ValueError, match="attn_dropout"):
        M.TransformerEncoderLayer(136, 2, 272, attn_dropout=0.1)
    with pytest.raises(ValueError, match="nhead"):
        M.TransformerEncoderLayer(136, 3, 272)
    with pytest.raises(ValueError, match="nhead"):
        M.TransformerEncoderLayer(274, 1, 272)                      # head width 274
    with pytest.raises(ValueError, match="num_layers"):
        M.TransformerEncoder(M.TransformerEncoderLayer(136, 2, 272), 0)
    enc = M.TransformerEncoder(M.TransformerEncoderLayer(136, 2, 272), 2)           # the issue's own construction
    assert len(enc.state_dict()) == 24
    with pytest.raises(NotImplementedError):
        enc(torch.zeros(4, 1, 136), mask=torch.zeros(4, 4))


# ---- the C entry points, host side ----------------------------------------------------------------------------------------------
def test_supported_truth_table():
    L = hip.lib()
    assert L.otp_token_attn_supported(136, 1, 200) == 1             # hd = 136
    assert L.otp_token_attn_supported(137, 1, 200) == 0             # hd = 137
    assert L.otp_token_attn_supported(272, 2, 6912) == 1 and L.otp_token_attn_supported(274, 2, 6912) == 0
    assert L.otp_token_attn_supported(136, 3, 200) == 0             # C % nh != 0
    assert L.otp_token_attn_supported(136, 2, 0) == 0               # T = 0
    assert L.otp_token_attn_supported(5, 1, 1) == 1 and L.otp_token_attn_supported(17, 1, 35) == 1
    assert L.otp_token_attn_supported(0, 1, 5) == 0 and L.otp_token_attn_supported(16, 0, 5) == 0


@pytest.mark.parametrize("b,nh,t,hd", [(16, 2, 6912, 68), (1, 1, 1, 1), (2, 8, 333, 17)])
def test_workspace_does_not_grow_with_t_squared(b, nh, t, hd):
    n = hip.lib().otp_token_attn_workspace(b, nh, t, hd)
    assert 0 < n <= 16 * b * nh * t + 4096


def test_entry_points_return_bad_arg_on_null_pointers():
    L = hip.lib()
    assert L.otp_token_attn_forward(None, None, None, None, None, None, 1, 16, 2, 8, 1.0, None) == -1
    assert L.otp_token_attn_backward(None, None, None, None, None, None, None, None, None, None, None, 1, 16, 2, 8, 1.0, None) == -1
    assert L.otp_token_attn_map(None, None, None, None, None, 1, 16, 2, 8, 1.0, None) == -1


def test_python_face_validates_before_any_launch():
    """CPU tensors: every ValueError below is raised before the GPU is asked for anything."""
    q = torch.zeros(2, 34, 16)
    with pytest.raises(ValueError, match="heads"):
        TA.token_attn(q, q, q, 3, 1.0)
    with pytest.raises(ValueError, match="head width"):
        TA.token_attn(torch.zeros(1, 274, 4), torch.zeros(1, 274, 4), torch.zeros(1, 274, 4), 1, 1.0)
    with pytest.raises(ValueError, match="contiguous"):
        TA.token_attn(q[:, :, ::2], q[:, :, ::2], q[:, :, ::2], 2, 1.0)
    with pytest.raises(ValueError, match="float32"):
        TA.token_attn(q.double(), q.double(), q.double(), 2, 1.0)
    with pytest.raises(ValueError, match="key_padding_mask"):
        TA.token_attn(q, q, q, 2, 1.0, torch.zeros(2, 15, dtype=torch.bool))
    with pytest.raises(ValueError, match="key_padding_mask"):
        TA.token_attn(q, q, q, 2, 1.0, torch.zeros(2, 16, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        TA.token_attn(q, q, q, 2, 1.0)                              # well-formed, but on the CPU


# ---- the OTPose extension keys ------------------------------------------------------------------------------------------------------
def _keyed_cfg(**keys):
    from otpose_amd import tiny_cfg
    cfg = tiny_cfg(8, (64, 96))
    for k, v in keys.items():
        cfg.MODEL[k] = v
    return cfg


def test_default_model_keeps_its_state_dict_keys():
    from otpose_amd import OTPose, tiny_cfg
    base = set(OTPose(tiny_cfg(8, (64, 96))).state_dict())
    assert not [k for k in base if k.startswith(("token_encoder", "flow_token_encoder", "temporal_pos_embedding",
                                                 "flow_pos_embedding"))]
    zeros = _keyed_cfg(TOKEN_LAYERS=0, FLOW_TOKEN_LAYERS=0, TOKEN_HEADS=2, TOKEN_PRE_NORM=False, TOKEN_PE="sine")
    assert set(OTPose(zeros).state_dict()) == base


@pytest.mark.parametrize("pe", ["sine", "learnable", "none"])
def test_keys_add_exactly_the_encoders_and_the_tables(pe):
    from otpose_amd import OTPose, tiny_cfg
    base = set(OTPose(tiny_cfg(8, (64, 96))).state_dict())
    m = OTPose(_keyed_cfg(TOKEN_LAYERS=2, FLOW_TOKEN_LAYERS=1, TOKEN_PE=pe, TOKEN_PRE_NORM=True))
    extra = set(m.state_dict()) - base
    assert base <= set(m.state_dict())
    tables = {"sine": {"temporal_pos_embedding"}, "learnable": {"temporal_pos_embedding", "flow_pos_embedding"}, "none": set()}[pe]
    assert {k for k in extra if "." not in k} == tables            # 'sine': no flow table, width 17 has no sine table
    assert {k.split(".")[0] for k in extra if "." in k} == {"token_encoder1", "token_encoder2", "flow_token_encoder"}
    d, j, t = m.temporal_encoding_dim, m.patch_dim, m.num_patches
    assert len(m.token_encoder1.layers) == 2 and len(m.flow_token_encoder.layers) == 1
    assert m.token_encoder1.layers[0].linear1.weight.shape == (2 * d, d) and m.token_encoder1.layers[0].nhead == 2
    assert m.flow_token_encoder.layers[0].linear1.weight.shape == (2 * j, j) and m.flow_token_encoder.layers[0].nhead == 1
    assert m.token_encoder2.layers[1].normalize_before
    if pe != "none":
        assert m.temporal_pos_embedding.shape == (1, t, d)
        assert m.temporal_pos_embedding.requires_grad == (pe == "learnable")
    if pe == "sine":
        assert torch.equal(m.temporal_pos_embedding, TA.sine_position_embedding(m.pe_h, m.pe_w, d))


@pytest.mark.parametrize("key,value", [("TOKEN_LAYERS", -1), ("TOKEN_LAYERS", 1.0), ("TOKEN_LAYERS", True), ("FLOW_TOKEN_LAYERS", -2),
                                       ("FLOW_TOKEN_LAYERS", "1"), ("TOKEN_HEADS", 3), ("TOKEN_HEADS", 0), ("TOKEN_HEADS", 2.0),
                                       ("TOKEN_FFN", 0), ("TOKEN_FFN", 64.0), ("TOKEN_PRE_NORM", 1), ("TOKEN_PE", "cosine"),
                                       ("TOKEN_PE", None)])
def test_malformed_key_values_raise_naming_the_key(key, value):
    """Rejected also with no layer asked for: a bad key does not wait for the day a layer is."""
    from otpose_amd import OTPose
    with pytest.raises(ValueError, match="MODEL." + key):
        OTPose(_keyed_cfg(**{key: value}))


def test_head_width_above_the_kernel_limit_raises():
    from otpose_amd import OTPose, tiny_cfg
    cfg = tiny_cfg(8, (64, 96))
    cfg.MODEL.NUM_JOINTS, cfg.MODEL.TOKEN_HEADS = 18, 1             # token width 18 * 8 = 144 in one head
    with pytest.raises(ValueError, match="MODEL.TOKEN_HEADS"):
        OTPose(cfg)


def test_make_optimizer_covers_the_new_parameters():
    from otpose_amd import OTPose
    from otpose_amd import optim
    cfg = _keyed_cfg(TOKEN_LAYERS=1, FLOW_TOKEN_LAYERS=1, TOKEN_PE="learnable")
    m = OTPose(cfg)
    groups = optim.reference_param_groups(m, cfg)
    names = {id(p): n for n, p in m.named_parameters()}
    decay, no_decay, pretrained = ({names[id(p)] for p in g["params"]} for g in groups)
    assert decay | no_decay | pretrained == set(names.values())
    new = [n for n in names.values() if n.startswith(("token_encoder", "flow_token_encoder", "temporal_pos", "flow_pos"))]
    assert len(new) == 3 * 12 + 2
    for n in new:
        heavy = n.endswith(("in_proj_weight", "out_proj.weight", "linear1.weight", "linear2.weight"))
        assert (n in decay) == heavy and (n in no_decay) == (not heavy), n
    assert groups[1]["weight_decay"] == 0.0
