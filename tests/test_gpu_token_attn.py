"""Token x token attention on the GPU (csrc/tokattn.hip, otpose_amd/token_attn.py): the bare operator, its backward and the
attention map against the float64 restatement of tests/token_attn_ref.py.

Bounds: ``reductions_cases.bound(yardstick, ref, cap)`` - four times the error of the fp32 restatement on the same operands, at
least 4 ulp of the reference's maximum, never above cap * max(1, max|ref|); cap 3e-5 forward, 1e-4 gradients (the caps of
tests/test_gpu_local_attn.py).  Every comparison prints a ``TOKATTN|`` line with the error beside the yardstick.

The kernels walk 64-token tiles on both sides, so the largest shape (T = 1030) spans 17 key tiles and 17 query tiles, the last
of them partial.  Mask cases: scattered keys, the FIRST key tile wholly masked, a wholly masked middle tile (the edge cases of
the running maximum); every sample keeps at least one live key - all keys masked is outside the operator's contract.

Modules: the golden cases (a), (b), (c) of tests/golden/token_encoder.npz through ``modules.TransformerEncoder`` against the
float64 restatement (which tests/test_token_attn_host.py ties to the reference's outputs), cap 1e-4: the module's projections
run in exact fp32, not on split products.

Model: the tiny OTPose with ``TOKEN_LAYERS = 1`` / ``FLOW_TOKEN_LAYERS = 1`` through the inference engine (eagerly and under its
hipGraph) against the oracle's forward with the restated token encoders put in front of its ConvTransformers, and one training
step against fp64 autograd of that restatement."""
import functools
import math
import os

import numpy as np
import pytest
import torch
from torch import nn

from otpose_amd import modules as M
from otpose_amd import token_attn as TA
from tests import reductions_cases as K
from tests import token_attn_ref as R
from tests.conftest import seeded

pytestmark = pytest.mark.gpu
D = torch.float64
TILE = 64
# (B, C, n_head, T)
SHAPES = [(1, 5, 1, 5), (2, 17, 1, 35), (2, 136, 2, 108), (1, 136, 1, 200), (2, 136, 8, 432), (1, 204, 2, 333), (1, 64, 2, 1030)]
MASKS = ["none", "scattered", "first_tile", "middle_tile"]


def _check(name, got, ref, yard, cap):
    err, y = K.max_err(got, ref), K.max_err(yard, ref)
    b = K.bound(y, ref, cap)
    print(f"TOKATTN|{name}|err {err:.3e}|yardstick {y:.3e}|bound {b:.3e}|max|ref| {float(ref.abs().max()):.3e}")
    assert err <= b, f"{name}: error {err:.3e} above bound {b:.3e} (fp32 yardstick {y:.3e})"


def make_mask(kind, b, t, seed):
    """(B, T) bool, True = padding, or None.  A tile case needs a live key outside the tile; a shape too short for it takes the
    scattered mask instead (the test ids stay, the short shapes have a single tile)."""
    if kind == "none":
        return None
    mask = torch.zeros(b, t, dtype=torch.bool)
    if kind == "first_tile" and t > TILE:
        mask[:, :TILE] = True
    elif kind == "middle_tile" and t > 3 * TILE:
        mask[:, TILE:2 * TILE] = True
        mask[0, 2 * TILE + 3] = True
    else:
        g = torch.Generator().manual_seed(seed)
        mask = torch.rand(b, t, generator=g) < 0.3
        mask[:, int(torch.randint(t, (1,), generator=g))] = False
    assert bool((~mask).any(dim=1).all()), "every sample keeps a live key"
    return mask


@functools.lru_cache(maxsize=None)
def _case(b, c, nh, t, kind, qscale=1.0):
    """Operands, the float64 reference and the fp32 yardstick (forward and gradients) of one case, computed once."""
    seed = 11 * t + c + nh
    q, k, v, go = (seeded((b, c, t), seed + i) for i in range(4))
    q = q * qscale
    mask = make_mask(kind, b, t, seed + 5)
    scale = 1.0 / math.sqrt(c // nh)
    fn = lambda q_, k_, v_: R.token_attn(q_, k_, v_, nh, scale, mask)          # noqa: E731
    ref = R.autograd(fn, [q.double(), k.double(), v.double()], go.double())
    yard = R.autograd(fn, [q, k, v], go)
    return (q, k, v, go, mask, scale), ref, yard


def _dev(x):
    return None if x is None else x.cuda()


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_token_attn_forward_vs_fp64(shape, kind):
    (q, k, v, _, mask, scale), (ref, _), (yard, _) = _case(*shape, kind)
    with torch.no_grad():
        out = TA.token_attn(q.cuda(), k.cuda(), v.cuda(), shape[2], scale, _dev(mask))
    _check(f"fwd {shape} mask={kind}", out, ref, yard, 3e-5)


@pytest.mark.parametrize("kind", ["none", "first_tile"])
def test_token_attn_softmax_subtracts_the_maximum(kind):
    shape = (2, 136, 2, 108) if kind == "none" else (1, 64, 2, 1030)
    (q, k, v, _, mask, scale), (ref, _), (yard, _) = _case(*shape, kind, 40.0)
    b, c, nh, t = shape
    s = torch.einsum("bhci,bhcj->bhij", q.double().reshape(b, nh, c // nh, t), k.double().reshape(b, nh, c // nh, t)) * scale
    if mask is not None:                                            # only scores the kernel exponentiates count
        s = s.masked_fill(mask.reshape(b, 1, 1, t), float("-inf"))
    assert float(s.max()) > 89.0, "the scaled scores of live keys must overflow exp() in fp32 for this test to mean anything"
    with torch.no_grad():
        out = TA.token_attn(q.cuda(), k.cuda(), v.cuda(), nh, scale, _dev(mask))
    assert bool(torch.isfinite(out).all())
    _check(f"fwd q x40 {shape} mask={kind}", out, ref, yard, 3e-5)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_token_attn_backward_vs_fp64_and_deterministic(shape, kind):
    (q, k, v, go, mask, scale), (ref, gref), (yard, gyard) = _case(*shape, kind)

    def run():
        leaves = [x.cuda().requires_grad_() for x in (q, k, v)]
        out = TA.token_attn(*leaves, shape[2], scale, _dev(mask))
        out.backward(go.cuda())
        return out.detach(), [x.grad for x in leaves]
    out, grads = run()
    _check(f"train fwd {shape} mask={kind}", out, ref, yard, 3e-5)
    for name, g, r, y in zip(("dq", "dk", "dv"), grads, gref, gyard):
        _check(f"{name} {shape} mask={kind}", g, r, y, 1e-4)
    if mask is not None:
        dead = mask.cuda()[:, None, :].expand_as(grads[1])
        assert bool((grads[1][dead] == 0).all()) and bool((grads[2][dead] == 0).all()), "masked keys receive exactly zero dk / dv"
    out2, grads2 = run()
    assert torch.equal(out, out2)
    for g, g2 in zip(grads, grads2):
        assert torch.equal(g, g2)
    with torch.no_grad():                                           # the no-grad launch (no lse) and the Function's forward
        assert torch.equal(TA.token_attn(q.cuda(), k.cuda(), v.cuda(), shape[2], scale, _dev(mask)), out)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_token_attn_map_vs_fp64(shape, kind):
    (q, k, _, _, mask, scale), _, _ = _case(*shape, kind)
    nh = shape[2]
    ref = R.token_attn_map(q.double(), k.double(), nh, scale, mask)
    yard = R.token_attn_map(q, k, nh, scale, mask)
    got = TA.token_attn_map(q.cuda(), k.cuda(), nh, scale, _dev(mask))
    assert not got.requires_grad
    _check(f"map {shape} mask={kind}", got, ref, yard, 3e-5)
    rows = got.sum(dim=2)
    assert float((rows - 1).abs().max()) <= 1e-5, float((rows - 1).abs().max())
    if mask is not None:
        assert bool((got[mask.cuda()[:, None, :].expand_as(got)] == 0).all()), "masked columns are exactly zero"
    assert torch.equal(got, TA.token_attn_map(q.cuda(), k.cuda(), nh, scale, _dev(mask)))


def test_token_attn_rejects_unsupported_shapes_and_operands():
    q = torch.zeros(1, 274, 16, device="cuda")
    with pytest.raises(ValueError):
        TA.token_attn(q, q, q, 1, 1.0)                              # head width 274
    with pytest.raises(ValueError):
        TA.token_attn(q, q, q, 3, 1.0)                              # 274 % 3 != 0
    q = torch.zeros(2, 34, 16, device="cuda")
    with pytest.raises(ValueError):
        TA.token_attn(q.transpose(1, 2), q.transpose(1, 2), q.transpose(1, 2), 2, 1.0)      # not contiguous
    with pytest.raises(ValueError):
        TA.token_attn(q[:, :, ::2], q[:, :, ::2], q[:, :, ::2], 2, 1.0)
    with pytest.raises(ValueError):
        TA.token_attn(q.double(), q.double(), q.double(), 2, 1.0)
    with pytest.raises(ValueError):
        TA.token_attn(q, q, q, 2, 1.0, torch.zeros(2, 15, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError):
        TA.token_attn(q, q, q, 2, 1.0, torch.zeros(2, 16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        TA.token_attn_map(q, q[:, :, ::2], 2, 1.0)
    with pytest.raises(ValueError):
        TA.token_attn(q[:, :, :0].contiguous(), q[:, :, :0].contiguous(), q[:, :, :0].contiguous(), 2, 1.0)     # T = 0


# ---- modules against the reference's cases ---------------------------------------------------------------------------------------
# tag -> (E, heads, FFN, activation, pre-norm, layers, final norm, pe_only_at_begin, maps): tests/golden/make_golden_token_encoder.py
MODULE_CASES = {"a": (136, 2, 272, "gelu", False, 2, False, False, False), "b": (17, 1, 34, "relu", True, 2, True, False, True),
                "c": (136, 2, 272, "gelu", False, 2, False, True, False)}
MODULE_SEED = {"a": 10, "b": 40, "c": 10}


def _module(tag, maps=None):
    e, nh, ffn, act, pre, layers, norm, pe_begin, want_maps = MODULE_CASES[tag]
    want_maps = want_maps if maps is None else maps
    enc = M.TransformerEncoder(M.TransformerEncoderLayer(e, nh, ffn, activation=act, normalize_before=pre), layers,
                               nn.LayerNorm(e) if norm else None, pe_begin, want_maps)
    return R.fill_encoder_(enc, MODULE_SEED[tag])


@functools.lru_cache(maxsize=None)
def _module_case(tag):
    """Inputs of a golden case, the float64 restatement (tied to the reference by tests/test_token_attn_host.py) and its fp32
    run, computed once."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_encoder.npz"))
    e, nh, ffn, act, pre, layers, norm, pe_begin, _ = MODULE_CASES[tag]
    x, pos = torch.from_numpy(z[tag + "_x"]), torch.from_numpy(z[tag + "_pos"])
    mask = torch.from_numpy(z[tag + "_mask"]) if tag + "_mask" in z.files else None
    if mask is not None:
        assert bool((~mask).any(dim=1).all()), "every sample keeps a live key"
    sd = {k: v for k, v in _module(tag).state_dict().items()}
    run = lambda dt: R.encoder({k: v.to(dt) for k, v in sd.items()}, x.to(dt), layers, nh, act, pre, mask, pos.to(dt),   # noqa: E731
                               pe_begin)
    return (x, pos, mask), run(D), run(torch.float32)


@pytest.mark.parametrize("tag", sorted(MODULE_CASES))
def test_encoder_module_matches_fp64_restatement(tag):
    """The projections run in exact fp32 (the module switches the split-product route off), so the cap is 1e-4."""
    (x, pos, mask), (yr, mr), (yy, my) = _module_case(tag)
    enc = _module(tag, maps=True).cuda().eval()
    with torch.no_grad():
        y, maps = enc(x.cuda(), src_key_padding_mask=_dev(mask), pos=pos.cuda())
        y_only = _module(tag, maps=False).cuda().eval()(x.cuda(), src_key_padding_mask=_dev(mask), pos=pos.cuda())
    _check(f"module {tag} y", y, yr, yy, 1e-4)
    _check(f"module {tag} maps", maps, mr, my, 1e-4)
    assert maps.shape == (MODULE_CASES[tag][5], x.shape[1], x.shape[0], x.shape[0])
    assert torch.equal(y, y_only)
    if mask is not None:
        assert bool((maps[:, mask.cuda()[:, None, :].expand(maps.shape[1:])] == 0).all())


@pytest.mark.parametrize("tag", ["a", "b"])
def test_encoder_module_trains_like_fp64_autograd(tag):
    (x, pos, mask), _, _ = _module_case(tag)
    e, nh, ffn, act, pre, layers, norm, pe_begin, _ = MODULE_CASES[tag]
    go = seeded(tuple(x.shape), 77)
    sd = _module(tag).state_dict()

    def reference(dt):
        leaves = {k: v.detach().clone().to(dt).requires_grad_() for k, v in sd.items()}
        xl = x.detach().clone().to(dt).requires_grad_()              # a copy: the cached input stays unchanged
        y, _ = R.encoder(leaves, xl, layers, nh, act, pre, mask, pos.to(dt), pe_begin)
        y.backward(go.to(dt))
        return y.detach(), xl.grad, {k: v.grad for k, v in leaves.items()}
    yr, gxr, gr = reference(D)
    yy, gxy, gy = reference(torch.float32)

    def step():
        enc = _module(tag, maps=False).cuda().train()
        for layer in enc.layers:
            layer.p_drop = 0.0
        xg = x.detach().cuda().requires_grad_()
        y = enc(xg, src_key_padding_mask=_dev(mask), pos=pos.cuda())
        y.backward(go.cuda())
        return y.detach(), xg.grad, {k: p.grad for k, p in enc.named_parameters()}
    y, gx, grads = step()
    _check(f"module train {tag} y", y, yr, yy, 1e-4)
    _check(f"module train {tag} dx", gx, gxr, gxy, 1e-4)
    assert sorted(grads) == sorted(gr)
    for k, g in grads.items():
        assert g is not None, k
        _check(f"module train {tag} d{k}", g, gr[k], gy[k], 1e-4)
    y2, gx2, grads2 = step()
    assert torch.equal(y, y2) and torch.equal(gx, gx2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k


def test_encoder_module_deviations_raise():
    enc = _module("b").cuda().eval()
    x = torch.zeros(35, 2, 17, device="cuda")
    with pytest.raises(NotImplementedError):
        enc(x, mask=torch.zeros(35, 35, device="cuda"))
    with pytest.raises(ValueError):
        enc(x, src_key_padding_mask=torch.zeros(2, 34, dtype=torch.bool, device="cuda"))


# ---- the tiny OTPose with the extension keys --------------------------------------------------------------------------------------
NAMES = ("output", "rough", "intersection", "prev_b", "context", "squeezed", "total_b")
ENCODERS = {"temporal_encoder1": ("token_encoder1", "temporal_pos_embedding"),
            "temporal_encoder2": ("token_encoder2", "temporal_pos_embedding"),
            "flow_encoder": ("flow_token_encoder", "flow_pos_embedding")}


def _token_cfg(pre=False):
    from otpose_amd import tiny_cfg
    cfg = tiny_cfg(8, (64, 96))
    cfg.MODEL.TOKEN_LAYERS, cfg.MODEL.FLOW_TOKEN_LAYERS, cfg.MODEL.TOKEN_PRE_NORM = 1, 1, pre
    return cfg


def _token_model(pre=False):
    from otpose_amd import OTPose
    from otpose_amd import synthetic as S
    cfg = _token_cfg(pre)
    m = OTPose(cfg)
    # the synthetic recipe sees the key set WITHOUT the new keys (it draws what it draws for the default model); the encoders get
    # the seeded fill of tests/token_attn_ref.py, the sine table stays as built
    sd = m.state_dict()
    new = ("token_encoder", "flow_token_encoder", "temporal_pos_embedding", "flow_pos_embedding")
    vals = S.synthetic_state_dict({k: tuple(v.shape) for k, v in sd.items() if not k.startswith(new)}, S.WEIGHT_SEED,
                                  S.gains_for(cfg))
    with torch.no_grad():
        for k, v in vals.items():
            sd[k].copy_(v.to(sd[k].dtype))
    for i, name in enumerate(("token_encoder1", "token_encoder2", "flow_token_encoder")):
        R.fill_encoder_(getattr(m, name), 100 + 30 * i)
    return m, cfg


def _restated_forward(sd, cfg, x, margin, training_bn=False):
    """oracle.otpose_forward with the token encoders of tests/token_attn_ref.py in front of the three ConvTransformers: on the
    input plus the ConvTransformer's own positional table, which the ConvTransformer then does not add again."""
    from oracle import otpose_oracle as O
    plain = O.conv_transformer

    def conv_transformer(sd_, p, x4, n_head, arch):
        name, pos_name = ENCODERS[p]
        b, c, h, w = x4.shape
        t = h * w
        x = x4.reshape(b, c, t) + sd_[p + ".pos_embd"][:, :, :t]
        sub = {k[len(name) + 1:]: v for k, v in sd_.items() if k.startswith(name + ".")}
        pos = sd_[pos_name].permute(1, 0, 2) if pos_name in sd_ else None
        pre = cfg.MODEL.TOKEN_PRE_NORM
        y, _ = R.encoder(sub, x.permute(2, 0, 1), 1, 2 if c > 17 else 1, "gelu", pre, None, pos)
        zero = dict(sd_)
        zero[p + ".pos_embd"] = torch.zeros_like(sd_[p + ".pos_embd"])
        return plain(zero, p, y.permute(1, 2, 0).reshape(b, c, h, w), n_head, arch)
    O.conv_transformer = conv_transformer
    try:
        return O.otpose_forward(sd, cfg, x, margin, training_bn)
    finally:
        O.conv_transformer = plain


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("pre", [False, True])
def test_tiny_otpose_with_token_encoders_matches_restatement(monkeypatch, graph, pre):
    """The criterion of tests/test_gpu_e2e.py::test_e2e_tiny_matches_reference_golden (1e-3 relative to max(1, max|ref|), the
    engine's projections run on its usual routes), eagerly and under the engine's hipGraph, whose replay must be bit-identical."""
    from otpose_amd import synthetic as S
    monkeypatch.setenv("OTPOSE_HIP_GRAPH", graph)
    m, cfg = _token_model(pre)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
    with torch.no_grad():
        ref = _restated_forward(sd, cfg, x, margin)
        m = m.cuda().eval()
        outs = [o.cpu() for o in m(x.cuda(), margin=margin.cuda())]
        again = [o.cpu() for o in m(x.cuda(), margin=margin.cuda())]
        third = [o.cpu() for o in m(x.cuda(), margin=margin.cuda())]
    assert (m._engine.graph is not None) == (graph == "1")
    assert sum(1 for _ in m.token_encoder1.parameters()) == 12
    for n, o, r in zip(NAMES, outs, ref):
        assert o.shape == r.shape, n
        err = float((o - r).abs().max())
        print(f"TOKATTN|e2e graph={graph} pre={pre} {n}|err {err:.3e}|max|ref| {float(r.abs().max()):.3e}")
        assert err <= 1e-3 * max(1.0, float(r.abs().max())), f"{n}: max abs err {err}"
    for a, b, c in zip(outs, again, third):
        assert torch.equal(a, b) and torch.equal(b, c)


def test_token_encoders_change_the_output_and_the_fp16_engine_refuses_them():
    from otpose_amd import OTPose, tiny_cfg
    from otpose_amd import synthetic as S
    m, cfg = _token_model()
    x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
    base = OTPose(tiny_cfg(8, (64, 96)))
    base.load_state_dict({k: v for k, v in m.state_dict().items() if k in base.state_dict()})
    with torch.no_grad():
        a = m.cuda().eval()(x.cuda(), margin=margin.cuda())[0]
        b = base.cuda().eval()(x.cuda(), margin=margin.cuda())[0]
    assert float((a - b).abs().max()) > 1e-4
    from otpose_amd.engine_h16 import InferenceEngineH16
    with pytest.raises(ValueError, match="TOKEN_LAYERS"):
        InferenceEngineH16(m, 1, "cuda")


def test_tiny_otpose_with_token_encoders_trains():
    """One training step: the gradients of the new parameters against fp64 autograd of the restatement with batch statistics
    (bound: 4 x the fp32 restatement's error, cap 1e-4 relative to max(1, max|ref|)); a second step is bit-identical."""
    from otpose_amd import synthetic as S
    from otpose_amd import train as TR
    from oracle import otpose_oracle as O
    m, cfg = _token_model()
    x, margin = S.synthetic_clip(2, cfg.MODEL.IMAGE_SIZE)
    tgt, wt = S.synthetic_targets(2, tuple(cfg.MODEL.HEATMAP_SIZE), cfg.MODEL.NUM_JOINTS, sigma=1.5, seed=77)
    new = [n for n, p in m.named_parameters() if n.startswith(("token_encoder", "flow_token_encoder")) and p.requires_grad]
    assert len(new) == 36

    def reference(dt):
        sd = {k: v.detach().clone().to(dt) if v.is_floating_point() else v.clone() for k, v in m.state_dict().items()}
        for n in new:
            sd[n].requires_grad_()
        outs = _restated_forward(sd, cfg, x.to(dt), margin.to(dt), True)
        loss = O.joint_mse_loss(outs[0], tgt.to(dt), wt.to(dt))
        return loss.detach(), dict(zip(new, torch.autograd.grad(loss, [sd[n] for n in new])))
    lr, gr = reference(D)
    ly, gy = reference(torch.float32)

    def step():
        mm, _ = _token_model()
        mm = mm.cuda().train()
        mm.train_dropout = False
        outs = TR.forward_train(mm, x.cuda(), margin.cuda())
        loss = O.joint_mse_loss(outs[0], tgt.cuda(), wt.cuda())
        loss.backward()
        return loss.detach(), {n: p.grad.clone() for n, p in mm.named_parameters() if n in new}
    loss, grads = step()
    _check("model train loss", loss, lr, ly, 1e-4)
    for n in new:
        assert float(gr[n].abs().max()) > 0, n
        _check(f"model train d{n}", grads[n], gr[n], gy[n], 1e-4)
    loss2, grads2 = step()
    assert torch.equal(loss, loss2)
    for n in new:
        assert torch.equal(grads[n], grads2[n]), n
