"""Token attention with half products on the GPU (csrc/tokattn_h.hip, ``token_attn(products="half")``).

References: the exact float64 operator of tests/token_attn_ref.py and the rounded restatement of tests/token_attn_half_ref.py.
Two bounds, both fixed before any kernel ran:

  a-priori   |o - o_fp64| <= (exp(2 delta) - 1 + 3u) max|v| + 1e-6 with u = 2^-11 and delta = scale (2u + u^2) max_ij sum_c |q_ci| |k_cj|
             over live keys, per case from its own operands (``token_attn_half_ref.forward_bound``)
  yardstick  error against the reference <= 4 x the error of the rounded restatement evaluated in torch fp32 on the GPU against the
             same reference, with a floor of 4 half-ulps (4 * 2^-11) of max|ref|

Every comparison prints a ``TOKATTN_H|`` line.  Shapes are the smallest at which a path of the kernel is taken for the first time
(partial / exact / one-past key tiles, head widths at and one past a 16-channel block, the widest block, two heads)."""
import functools
import math
import os

import numpy as np
import pytest
import torch
from torch import nn

from otpose_amd import attn_dropout as AD
from otpose_amd import hip
from otpose_amd import modules as M
from otpose_amd import token_attn as TA
from tests import reductions_cases as K
from tests import token_attn_half_ref as H
from tests import token_attn_ref as R
from tests.conftest import seeded

pytestmark = pytest.mark.gpu
D = torch.float64
TILE = 64
# (B, C, n_head, T)
SHAPES = [(1, 1, 1, 1), (2, 34, 2, 63), (2, 34, 2, 64), (2, 34, 2, 65), (1, 16, 1, 130), (1, 17, 1, 35), (1, 136, 1, 200),
          (1, 272, 2, 70)]
MASKS = ["none", "first_tile", "all_but_one", "random"]
SEED = 0xC0FFEE0123456789


def bound(yard, ref):
    return max(4.0 * yard, 4.0 * H.U * float(ref.abs().max()))


def _check(name, got, ref, yard):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: inf or NaN"
    err, y = K.max_err(got, ref), K.max_err(yard, ref)
    b = bound(y, ref)
    print(f"TOKATTN_H|{name}|err {err:.3e}|yardstick {y:.3e}|bound {b:.3e}|max|ref| {float(ref.abs().max()):.3e}")
    assert err <= b, f"{name}: error {err:.3e} above bound {b:.3e} (fp32 rounded yardstick {y:.3e})"


def make_mask(kind, b, t, seed):
    """(B, T) bool, True = padding, or None when the case does not exist on this shape (first tile: T > 64; one key: T > 1)."""
    if kind == "none":
        return None
    mask = torch.zeros(b, t, dtype=torch.bool)
    g = torch.Generator().manual_seed(seed)
    if kind == "first_tile":
        if t <= TILE:
            return None
        mask[:, :TILE] = True
    elif kind == "all_but_one":
        if t == 1:
            return None
        mask[:] = True
        for i in range(b):
            mask[i, int(torch.randint(t, (1,), generator=g))] = False
    else:                                                           # random, the last (partial) tile ragged: its last key is padding
        if t == 1:
            return None
        mask = torch.rand(b, t, generator=g) < 0.4
        mask[:, t - 1] = True
        mask[:, int(torch.randint(t - 1, (1,), generator=g))] = False
    assert bool((~mask).any(dim=1).all()), "every sample keeps a live key"
    return mask


CASES = [(s, kind) for s in SHAPES for kind in MASKS if kind == "none" or make_mask(kind, s[0], s[3], 0) is not None]


def _dev(x):
    return None if x is None else x.cuda()


@functools.lru_cache(maxsize=None)
def _case(b, c, nh, t, kind):
    """Operands, the exact float64 reference, and the rounded restatement in fp32 on the GPU (forward and gradients), once."""
    seed = 13 * t + c + nh
    q, k, v, go = (seeded((b, c, t), seed + i) for i in range(4))
    v = v * 0.25                                                    # max|v| of order 1
    mask = make_mask(kind, b, t, seed + 5)
    scale = 1.0 / math.sqrt(c // nh)
    ref = R.autograd(lambda q_, k_, v_: R.token_attn(q_, k_, v_, nh, scale, mask), [q.double(), k.double(), v.double()], go.double())
    yo, yg = R.autograd(lambda q_, k_, v_: H.token_attn(q_, k_, v_, nh, scale, _dev(mask)), [q.cuda(), k.cuda(), v.cuda()], go.cuda())
    return (q, k, v, go, mask, scale), ref, (yo.cpu(), [g.cpu() for g in yg])


def _run(case, nh, **kw):
    q, k, v, go, mask, scale = case
    leaves = [x.cuda().requires_grad_() for x in (q, k, v)]
    out = TA.token_attn(*leaves, nh, scale, _dev(mask), products="half", **kw)
    out.backward(go.cuda())
    return out.detach(), [x.grad for x in leaves]


@pytest.mark.parametrize("shape,kind", CASES)
def test_forward_inside_the_a_priori_bound(shape, kind):
    (q, k, v, _, mask, scale), (ref, _), _ = _case(*shape, kind)
    with torch.no_grad():
        out = TA.token_attn(q.cuda(), k.cuda(), v.cuda(), shape[2], scale, _dev(mask), products="half")
    lim = H.forward_bound(q, k, v, shape[2], scale, mask)
    err = K.max_err(out, ref)
    print(f"TOKATTN_H|apriori {shape} mask={kind}|err {err:.3e}|bound {lim:.3e}|max|v| {float(v.abs().max()):.3e}")
    assert bool(torch.isfinite(out).all())
    assert err <= lim


@pytest.mark.parametrize("shape,kind", CASES)
def test_forward_and_gradients_by_the_yardstick_rule(shape, kind):
    case, (ref, gref), (yard, gyard) = _case(*shape, kind)
    mask = case[4]
    out, grads = _run(case, shape[2])
    _check(f"fwd {shape} mask={kind}", out, ref, yard)
    for name, g, r, y in zip(("dq", "dk", "dv"), grads, gref, gyard):
        _check(f"{name} {shape} mask={kind}", g, r, y)
    if mask is not None:
        dead = mask.cuda()[:, None, :].expand_as(grads[1])
        assert bool((grads[1][dead] == 0).all()) and bool((grads[2][dead] == 0).all()), "masked keys receive exactly zero dk / dv"
    out2, grads2 = _run(case, shape[2])
    assert torch.equal(out, out2)
    for g, g2 in zip(grads, grads2):
        assert torch.equal(g, g2)
    with torch.no_grad():                                           # the no-grad launch (no lse) and the Function's forward
        q, k, v, _, _, scale = case
        assert torch.equal(TA.token_attn(q.cuda(), k.cuda(), v.cuda(), shape[2], scale, _dev(mask), products="half"), out)


@pytest.mark.parametrize("shape,kind", [((2, 34, 2, 65), "random"), ((1, 136, 1, 200), "none")])
def test_gradients_keep_their_precision_for_a_tiny_cotangent(shape, kind):
    """A cotangent far below 2^-14, where a half is subnormal, as a mean-reduced loss hands it over - and one whose first query
    tile is 2^20 times larger than the rest, so that the accumulators of pass B move between the scales of two tiles.  The rule
    and its floor scale with the reference, so an error of the size of a subnormal half's spacing cannot pass."""
    b, c, nh, t = shape
    (q, k, v, go, mask, scale), _, _ = _case(*shape, kind)
    go = go * 2.0 ** -20
    go[:, :, :TILE] *= 2.0 ** 20
    go[:, :, TILE:] *= 2.0 ** -3
    _, gref = R.autograd(lambda q_, k_, v_: R.token_attn(q_, k_, v_, nh, scale, mask), [q.double(), k.double(), v.double()], go.double())
    _, gyard = R.autograd(lambda q_, k_, v_: H.token_attn(q_, k_, v_, nh, scale, _dev(mask)), [q.cuda(), k.cuda(), v.cuda()], go.cuda())
    _, grads = _run((q, k, v, go, mask, scale), nh)
    for name, g, r, y in zip(("dq", "dk", "dv"), grads, gref, gyard):
        _check(f"tiny cotangent {name} {shape} mask={kind}", g, r, y)
        late = (slice(None), slice(None), slice(TILE, None))        # dq of the small tiles alone: its own reference sets its floor
        if name == "dq":
            _check(f"tiny cotangent dq past the first tile {shape} mask={kind}", g[late], r[late], y[late])


def test_half_output_is_not_the_fp32_kernels():
    """The half kernel's output differs from the fp32 kernel's by more than the fp32 kernel's own error against fp64."""
    shape = (1, 136, 1, 200)
    (q, k, v, _, _, scale), (ref, _), _ = _case(*shape, "none")
    with torch.no_grad():
        exact = TA.token_attn(q.cuda(), k.cuda(), v.cuda(), 1, scale)
        half = TA.token_attn(q.cuda(), k.cuda(), v.cuda(), 1, scale, products="half")
    own, apart = K.max_err(exact, ref), float((half - exact).abs().max())
    print(f"TOKATTN_H|half vs f32 {shape}|apart {apart:.3e}|f32 kernel err {own:.3e}")
    assert apart > own and apart > 0


# ---- dropout: the mask the kernels apply -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.25, 0.5])
def test_dropout_mask_is_keep_mask_in_the_forward_and_in_pass_b(p):
    """hd = 136 >= T = 130 (three key tiles): with q = 0 every probability is 1 / T; v[c][j] = [c == j] makes out[c][i] the
    dropped P[i][c], and a cotangent dO[c][i] = [c == i] makes dv[c][j] the dropped P[c][j] as pass B sees it."""
    b, c, nh, t = 2, 136, 1, 130
    keep = AD.keep_mask(SEED, b * nh, t, t, p, "cuda").bool()
    eye = torch.zeros(b, c, t, device="cuda")
    eye[:, :t, :] = torch.eye(t, device="cuda")
    z = torch.zeros(b, c, t, device="cuda")
    leaves = [x.clone().requires_grad_() for x in (z, z, eye)]
    out = TA.token_attn(*leaves, nh, 1.0, None, dropout_p=p, seed=SEED, products="half")
    out.backward(eye)
    assert torch.equal(out[:, :t, :].transpose(1, 2) != 0, keep)                    # out[c][i] = P m [i][c]
    assert torch.equal(leaves[2].grad[:, :t, :] != 0, keep)                         # dv[c][j] = P m [c][j]
    thr = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    survivor = float(np.float32(65536.0) / np.float32(65536 - thr)) / t
    assert float((out[:, :t, :].transpose(1, 2)[keep] - survivor).abs().max()) <= 2 * H.U * survivor


@pytest.mark.parametrize("shape,kind", [((2, 34, 2, 65), "random"), ((1, 136, 1, 200), "first_tile")])
def test_dropout_gradients_by_the_yardstick_rule(shape, kind):
    """All three passes under one seed against the rounded restatement with the SAME mask: a pass that drew another mask is off
    by whole probabilities, not by roundings."""
    b, c, nh, t = shape
    p = 0.5
    (q, k, v, go, mask, scale), _, _ = _case(*shape, kind)
    keep = AD.keep_mask(SEED, b * nh, t, t, p, "cuda").reshape(b, nh, t, t)
    thr = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    factor = keep.double().cpu() * (65536.0 / (65536 - thr))
    ref, gref = R.autograd(lambda q_, k_, v_: H.token_attn(q_, k_, v_, nh, scale, mask, False, factor),
                           [q.double(), k.double(), v.double()], go.double())
    gpu_factor = factor.float().cuda()
    yard, gyard = R.autograd(lambda q_, k_, v_: H.token_attn(q_, k_, v_, nh, scale, _dev(mask), True, gpu_factor),
                             [q.cuda(), k.cuda(), v.cuda()], go.cuda())
    out, grads = _run((q, k, v, go, mask, scale), nh, dropout_p=p, seed=SEED)
    _check(f"drop fwd {shape} mask={kind}", out, ref, yard.cpu())
    for name, g, r, y in zip(("dq", "dk", "dv"), grads, gref, gyard):
        _check(f"drop {name} {shape} mask={kind}", g, r, y.cpu())
    out2, grads2 = _run((q, k, v, go, mask, scale), nh, dropout_p=p, seed=SEED)
    assert torch.equal(out, out2) and all(torch.equal(a, b_) for a, b_ in zip(grads, grads2))


# ---- range guard -------------------------------------------------------------------------------------------------------------------
def test_operand_beyond_a_halfs_range_is_flagged_and_the_next_call_is_clean():
    """A flagged value, not a fault: every index of the launch is as in a well-formed one."""
    (q, k, v, _, _, scale), (ref, _), (yard, _) = _case(2, 34, 2, 65, "none")
    L = hip.lib()
    torch.cuda.synchronize()
    L.otp_range_flag_read(1)                                        # whatever an earlier test of the process left
    bad = k.clone()
    bad[1, 20, 40] = 7e4
    with torch.no_grad():
        with pytest.raises(FloatingPointError, match="65504"):
            TA.token_attn(q.cuda(), bad.cuda(), v.cuda(), 2, scale, products="half")
        assert L.otp_range_flag_read(0) == 0                        # the raise cleared the sticky word
        # the entry point itself, the output in hand: the word is set and the poison launch fills the output with NaN
        qd, kd, vd = q.cuda(), bad.cuda(), v.cuda()
        out = torch.zeros_like(qd)
        hip.check(L.otp_token_attn_forward_h1(hip.ptr(qd), hip.ptr(kd), hip.ptr(vd), None, hip.ptr(out), None, 2, 34, 2, 65, scale,
                                              0.0, 0, None, hip.stream_of(qd)), "otp_token_attn_forward_h1")
        hip.check(L.otp_range_poison(hip.ptr(out), out.numel(), hip.stream_of(qd)), "otp_range_poison")
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
        assert L.otp_range_flag_read(1) == 12
        good = TA.token_attn(q.cuda(), k.cuda(), v.cuda(), 2, scale, products="half")
    assert L.otp_range_flag_read(0) == 0
    _check("fwd after a flagged call", good, ref, yard)
    leaves = [x.cuda().requires_grad_() for x in (q, k, v)]
    out = TA.token_attn(*leaves, 2, scale, products="half")
    with pytest.raises(FloatingPointError):
        out.backward(torch.full_like(out, 7e4))                     # the cotangent is an operand of the backward's products
    assert L.otp_range_flag_read(0) == 0


# ---- modules -----------------------------------------------------------------------------------------------------------------------
MODULE_CASES = {"a": (136, 2, 272, "gelu", False, 2, False, False), "b": (17, 1, 34, "relu", True, 2, True, False)}
MODULE_SEED = {"a": 10, "b": 40}


def _module(tag):
    e, nh, ffn, act, pre, layers, norm, pe_begin = MODULE_CASES[tag]
    layer = M.TransformerEncoderLayer(e, nh, ffn, activation=act, normalize_before=pre).set_products("half")
    return R.fill_encoder_(M.TransformerEncoder(layer, layers, nn.LayerNorm(e) if norm else None, pe_begin), MODULE_SEED[tag])


@pytest.mark.parametrize("tag", sorted(MODULE_CASES))
def test_encoder_module_with_half_products_matches_the_rounded_restatement(tag):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_encoder.npz"))
    e, nh, ffn, act, pre, layers, norm, pe_begin = MODULE_CASES[tag]
    x, pos = torch.from_numpy(z[tag + "_x"]), torch.from_numpy(z[tag + "_pos"])
    mask = torch.from_numpy(z[tag + "_mask"]) if tag + "_mask" in z.files else None
    enc = _module(tag)
    assert [l.products for l in enc.layers] == ["half"] * layers
    sd = enc.state_dict()
    run = lambda dt, rounding: H.encoder({k: v.to(dt) for k, v in sd.items()}, x.to(dt), layers, nh, act, pre, mask, pos.to(dt),   # noqa: E731
                                         pe_begin, rounding)[0]
    ref, yard, exact = run(D, True), run(torch.float32, True), run(D, False)
    with torch.no_grad():
        y = enc.cuda().eval()(x.cuda(), src_key_padding_mask=_dev(mask), pos=pos.cuda())
        y32 = _module(tag).cuda().eval()
        for layer in y32.layers:
            layer.set_products("f32")
        y32 = y32(x.cuda(), src_key_padding_mask=_dev(mask), pos=pos.cuda())
    _check(f"module {tag} y vs rounded fp64", y, ref, yard)
    print(f"TOKATTN_H|module {tag} y vs exact fp64|err {K.max_err(y, exact):.3e}|f32 module err {K.max_err(y32, exact):.3e}")
    assert not torch.equal(y, y32)


# ---- the tiny OTPose with MODEL.TOKEN_PRODUCTS ------------------------------------------------------------------------------------
def _model(products):
    """The tiny model of tests/test_gpu_token_attn.py (TOKEN_LAYERS = FLOW_TOKEN_LAYERS = 1) built with the key (None: absent)."""
    from otpose_amd import OTPose
    from tests.test_gpu_token_attn import _token_cfg, _token_model
    filled, _ = _token_model()
    cfg = _token_cfg()
    if products is not None:
        cfg.MODEL.TOKEN_PRODUCTS = products
    m = OTPose(cfg)
    m.load_state_dict(filled.state_dict())
    return m, cfg


def _eval_outputs(monkeypatch, products, graph):
    from otpose_amd import synthetic as S
    monkeypatch.setenv("OTPOSE_HIP_GRAPH", graph)
    m, cfg = _model(products)
    x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
    m = m.cuda().eval()
    with torch.no_grad():
        outs = [o.cpu() for o in m(x.cuda(), margin=margin.cuda())]
        again = [o.cpu() for o in m(x.cuda(), margin=margin.cuda())]
    assert (m._engine.graph is not None) == (graph == "1")
    m.check_range()
    for a, b in zip(outs, again):
        assert torch.equal(a, b)
    return outs


def test_tiny_otpose_half_products_eager_and_graph_and_against_f32(monkeypatch):
    from tests.test_gpu_token_attn import NAMES
    eager = _eval_outputs(monkeypatch, "half", "0")
    graph = _eval_outputs(monkeypatch, "half", "1")
    f32 = _eval_outputs(monkeypatch, "f32", "1")
    absent = _eval_outputs(monkeypatch, None, "1")
    moved = False
    for n, e, g, f, a in zip(NAMES, eager, graph, f32, absent):
        assert torch.equal(e, g), f"{n}: eager and hipGraph runs differ"
        assert torch.equal(f, a), f"{n}: TOKEN_PRODUCTS = 'f32' is not the model without the key"
        span = float(f.max() - f.min())
        err = float((e - f).abs().max())
        print(f"TOKATTN_H|e2e half vs f32 {n}|err {err:.3e}|range {span:.3e}|ratio {err / max(span, 1e-30):.3e}")
        assert err <= 8e-3 * span, f"{n}: {err:.3e} above 8e-3 of the range {span:.3e}"
        moved = moved or err > 0
    assert moved, "the half launches must change some bit of some output"


def test_engine_emits_the_half_launch_in_the_attention_slot():
    """The ten-launch layer keeps its other nine launches: same count, and only the attention's entry point differs."""
    from otpose_amd import synthetic as S
    counts = {}
    for products in ("f32", "half"):
        m, cfg = _model(products)
        x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
        m = m.cuda().eval()
        with torch.no_grad():
            m(x.cuda(), margin=margin.cuda())
        counts[products] = len(m._engine.ops)
    assert counts["half"] == counts["f32"]


def test_tiny_otpose_half_products_trains():
    """One training step: finite loss, the gradients of the token encoders' parameters by the yardstick rule against fp64 autograd
    of the model's restatement with the rounded attention; a second step is bit-identical.

    The cotangent that reaches the attention here is of the order of 1e-6 (a mean-reduced loss of 1e-2): without the per-tile power of
    two of backward pass A it lies in a half's subnormal range, and two of the 36 gradients then missed this rule at 5 x their
    yardstick."""
    from otpose_amd import synthetic as S
    from otpose_amd import train as TR
    from oracle import otpose_oracle as O
    from tests.test_gpu_token_attn import _restated_forward
    m, cfg = _model("half")
    x, margin = S.synthetic_clip(2, cfg.MODEL.IMAGE_SIZE)
    tgt, wt = S.synthetic_targets(2, tuple(cfg.MODEL.HEATMAP_SIZE), cfg.MODEL.NUM_JOINTS, sigma=1.5, seed=77)
    new = [n for n, p in m.named_parameters() if n.startswith(("token_encoder", "flow_token_encoder")) and p.requires_grad]
    assert len(new) == 36

    def reference(dt):
        sd = {k: v.detach().clone().to(dt) if v.is_floating_point() else v.clone() for k, v in m.state_dict().items()}
        for n in new:
            sd[n].requires_grad_()
        with H.rounded_attention():
            outs = _restated_forward(sd, cfg, x.to(dt), margin.to(dt), True)
        loss = O.joint_mse_loss(outs[0], tgt.to(dt), wt.to(dt))
        return loss.detach(), dict(zip(new, torch.autograd.grad(loss, [sd[n] for n in new])))
    lr, gr = reference(D)
    ly, gy = reference(torch.float32)

    def step():
        mm, _ = _model("half")
        mm = mm.cuda().train()
        mm.train_dropout = False
        outs = TR.forward_train(mm, x.cuda(), margin.cuda())
        loss = O.joint_mse_loss(outs[0], tgt.cuda(), wt.cuda())
        loss.backward()
        return loss.detach(), {n: p.grad.clone() for n, p in mm.named_parameters() if n in new}
    loss, grads = step()
    assert bool(torch.isfinite(loss))
    _check("model train loss", loss, lr, ly)
    loss2, grads2 = step()
    assert torch.equal(loss, loss2)
    for n in new:
        assert torch.equal(grads[n], grads2[n]), n
    misses = []
    for n in new:                                                   # every figure is printed before the rule is asserted
        try:
            _check(f"model train d{n}", grads[n], gr[n], gy[n])
        except AssertionError as e:
            misses.append(str(e))
    assert not misses, "\n".join(misses)
