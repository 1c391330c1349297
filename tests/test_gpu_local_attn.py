"""Local-window attention on the GPU (csrc/localattn.hip): the bare operator and its backward against the float64 restatement
of tests/local_attn_ref.py, the modules built on it against the reference's own outputs (tests/golden/local_attn.npz) through
the launches the inference engine emits, the tiny OTPose with the extension keys set, and the training graph.

Bounds: ``reductions_cases.bound(yardstick, ref, cap)`` - four times the error of the fp32 restatement on the same operands, at
least 4 ulp of the reference's maximum, never above cap * max(1, max|ref|); cap 3e-5 forward, 1e-4 gradients.  Every comparison
prints a ``LOCALATTN|`` line with the error beside the yardstick."""
import functools
import math

import pytest
import torch
from torch import nn

from otpose_amd import OTPose, ops, tiny_cfg
from otpose_amd import modules as M
from otpose_amd import synthetic as S
from otpose_amd import train as TR
from otpose_amd import train_ops as T
from tests import local_attn_ref as R
from tests import reductions_cases as K
from tests.conftest import seeded

pytestmark = pytest.mark.gpu
D = torch.float64
NAMES = ("output", "rough", "intersection", "prev_b", "context", "squeezed", "total_b")

# (B, C, n_head, T, window): the issue's six, then two whose T is no multiple of 4 (the word-by-word path of the kernels)
SHAPES = [(2, 34, 2, 4, 5), (2, 136, 2, 8, 9), (1, 17, 1, 36, 19), (2, 136, 2, 648, 9), (2, 136, 2, 648, 19),
          (2, 204, 2, 1056, 33), (1, 6, 1, 18, 7), (2, 14, 2, 90, 19)]


def _check(name, got, ref, yard, cap):
    err, y = K.max_err(got, ref), K.max_err(yard, ref)
    b = K.bound(y, ref, cap)
    print(f"LOCALATTN|{name}|err {err:.3e}|yardstick {y:.3e}|bound {b:.3e}|max|ref| {float(ref.abs().max()):.3e}")
    assert err <= b, f"{name}: error {err:.3e} above bound {b:.3e} (fp32 yardstick {y:.3e})"


@functools.lru_cache(maxsize=None)
def _case(b, c, nh, t, win, rel, qscale=1.0):
    """Operands, the float64 reference and the fp32 yardstick (forward and gradients) of one shape, computed once."""
    seed = 7 * t + win + c
    q, k, v, go = (seeded((b, c, t), seed + i) for i in range(4))
    q = q * qscale
    rp = seeded((1, 1, nh, win), seed + 9, 0.5) if rel else None
    scale = 1.0 / math.sqrt(c // nh)
    fn = lambda q_, k_, v_, r_: R.local_attn(q_, k_, v_, nh, win, scale, r_)          # noqa: E731
    dbl = [None if x is None else x.double() for x in (q, k, v, rp)]
    ref = R.autograd(fn, dbl, go.double())
    yard = R.autograd(fn, [q, k, v, rp], go)
    return (q, k, v, rp, go, scale), ref, yard


@pytest.mark.parametrize("rel", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_local_attn_forward_vs_fp64(shape, rel):
    b, c, nh, t, win = shape
    (q, k, v, rp, _, scale), (ref, _), (yard, _) = _case(*shape, rel)
    out = ops.local_attn(q.cuda(), k.cuda(), v.cuda(), nh, win, scale, None if rp is None else rp.cuda())
    _check(f"fwd {shape} rel={rel}", out, ref, yard, 3e-5)


def test_local_attn_softmax_subtracts_the_maximum():
    shape = (2, 136, 2, 648, 9)
    (q, k, v, rp, _, scale), (ref, _), (yard, _) = _case(*shape, True, 40.0)
    s = torch.einsum("bct,bct->bt", q.double(), k.double()) * scale
    assert float(s.max()) > 89.0, "the scaled scores must overflow exp() in fp32 for this test to mean anything"
    out = ops.local_attn(q.cuda(), k.cuda(), v.cuda(), 2, 9, scale, rp.cuda())
    assert bool(torch.isfinite(out).all())
    _check("fwd q x40", out, ref, yard, 3e-5)


@pytest.mark.parametrize("rel", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_local_attn_backward_vs_fp64_and_deterministic(shape, rel):
    b, c, nh, t, win = shape
    (q, k, v, rp, go, scale), (ref, gref), (yard, gyard) = _case(*shape, rel)

    def run():
        leaves = [x.cuda().requires_grad_() for x in (q, k, v)] + [None if rp is None else rp.cuda().requires_grad_()]
        out = T.local_attn(leaves[0], leaves[1], leaves[2], nh, win, scale, leaves[3])
        out.backward(go.cuda())
        return out.detach(), [None if x is None else x.grad for x in leaves]
    out, grads = run()
    _check(f"train fwd {shape} rel={rel}", out, ref, yard, 3e-5)
    for name, g, r, y in zip(("dq", "dk", "dv", "drel_pe"), grads, gref, gyard):
        if r is not None:
            _check(f"{name} {shape} rel={rel}", g, r, y, 1e-4)
    out2, grads2 = run()
    assert torch.equal(out, out2)
    for g, g2 in zip(grads, grads2):
        assert g is None or torch.equal(g, g2)


def test_local_attn_rejects_unsupported_shapes():
    q = torch.zeros(1, 34, 16, device="cuda")
    for win in (4, 3, 35):
        with pytest.raises(ValueError):
            ops.local_attn(q, q, q, 2, win, 1.0)
    with pytest.raises(ValueError):
        ops.local_attn(q[:, :, :12].contiguous(), q[:, :, :12].contiguous(), q[:, :, :12].contiguous(), 2, 9, 1.0)
    with pytest.raises(ValueError):
        T.local_attn(q, q, q, 2, 8, 1.0)


# ---- modules against the reference's outputs -----------------------------------------------------------------------------------
def _rel(g, tag):
    pre = tag + "_rel/"
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


def _close(got, ref, tol=5e-5):
    got = got.detach().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = float((got - ref).abs().max())
    print(f"LOCALATTN|golden|err {err:.3e}|max|ref| {float(ref.abs().max()):.3e}")
    assert err <= tol * max(1.0, float(ref.abs().max())), err


def _bare_engine(x):
    from otpose_amd.engine import InferenceEngine
    eng = InferenceEngine.bare("cuda")
    xin = eng.new(*x.shape)
    xin.copy_(x)
    eng.inp = xin
    return eng, xin


def _run(eng):
    torch.cuda.synchronize()
    eng._launch_all()
    torch.cuda.synchronize()


@pytest.mark.parametrize("tag,c,nh,win,stride", [("lmhca_136_s1", 136, 2, 9, 1), ("lmhca_136_s2", 136, 2, 9, 2),
                                                 ("lmhca_17_s1", 17, 1, 5, 1)])
def test_local_mhca_matches_golden(golden, tag, c, nh, win, stride):
    """dwconv + LayerNorm -> q / k / v projections -> the engine's attention dispatch -> proj."""
    g = golden("local_attn")
    mod = R.fill_windowed_(M.LocalMaskedMHCA(c, nh, win, stride, stride, proj_pdrop=0.1, use_rel_pe=True), 11, _rel(g, tag))
    x = g[tag + "_x"].cuda()
    dev = lambda p: p.detach().cuda().contiguous()          # noqa: E731
    qn, kn, vn = ops.dwconv_ln3(
        x, [dev(mod.query_conv.weight), dev(mod.key_conv.weight), dev(mod.value_conv.weight)],
        [dev(mod.query_norm.weight), dev(mod.key_norm.weight), dev(mod.value_norm.weight)],
        [dev(mod.query_norm.bias), dev(mod.key_norm.bias), dev(mod.value_norm.bias)], stride)
    lin = lambda m_, z: ops.conv2d(z.unsqueeze(2), dev(m_.weight), None, dev(m_.bias)).squeeze(2)   # noqa: E731
    q, k, v = lin(mod.query, qn), lin(mod.key, kn), lin(mod.value, vn)
    eng, _ = _bare_engine(x)
    att = eng.new(*q.shape)
    eng.attention(q, k, v, att, mod)
    _run(eng)
    assert len(eng.ops) == 1
    _close(lin(mod.proj, att), g[tag + "_y"])


@pytest.mark.parametrize("tag,c,nh,stride", [("ltblock_136_s1", 136, 2, 1), ("ltblock_136_s2", 136, 2, 2),
                                             ("ltblock_17_s1", 17, 1, 1)])
def test_windowed_transformer_block_matches_golden(golden, tag, c, nh, stride):
    """``InferenceEngine.tblock``: the generic block (C = 136) and the two-launch flow path (C = 17) around the local attention."""
    g = golden("local_attn")
    blk = R.fill_windowed_(M.TransformerBlock(c, nh, (stride, stride), 0.1, 0.1, 0.1, mha_win_size=9, use_rel_pe=True), 12,
                           _rel(g, tag)).eval()
    eng, xin = _bare_engine(g[tag + "_x"])
    with torch.no_grad():
        out = eng.tblock(blk, xin, stride)
    _run(eng)
    if c == 17:
        assert eng.routes.use_flow_fused and len(eng.ops) == 3          # flow_front, local attention, flow_back
    _close(out, g[tag + "_y"])


def test_windowed_conv_transformer_matches_golden(golden):
    g = golden("local_attn")
    ct = R.fill_windowed_(M.ConvTransformer(136, 136, 2, 3, 96, (0, 2, 2), h=12, proj_pdrop=0.1, path_pdrop=0.1,
                                            mha_win_size=[9, 9, 5], use_rel_pe=True), 14, _rel(g, "lct_136")).eval()
    x4 = g["lct_136_x"]
    b, c, h, w = x4.shape
    eng, xin = _bare_engine(x4.reshape(b, c, h * w) + ct.pos_embd[:, :, :h * w])
    stacked = eng.new(b, 3 * c, h * w)
    with torch.no_grad():
        eng.conv_transformer(ct, xin, stacked)
    _run(eng)
    for i in range(3):
        _close(stacked[:, i * c:(i + 1) * c], g[f"lct_136_y{i}"].reshape(b, c, h * w))


# ---- the tiny OTPose with the extension keys --------------------------------------------------------------------------------------
def _windowed_cfg():
    cfg = tiny_cfg(8, (64, 96))
    cfg.MODEL.MHA_WIN_SIZE, cfg.MODEL.USE_REL_PE = 9, True
    return cfg


def _windowed_model(g):
    cfg = _windowed_cfg()
    return R.fill_windowed_(OTPose(cfg), S.WEIGHT_SEED, _rel(g, "e2e")), cfg


@pytest.mark.parametrize("graph", ["1", "0"])
def test_tiny_otpose_with_windows_matches_reference(golden, monkeypatch, graph):
    """The criterion of tests/test_gpu_e2e.py::test_e2e_tiny_matches_reference_golden, with the captured hipGraph and without."""
    monkeypatch.setenv("OTPOSE_HIP_GRAPH", graph)
    g = golden("local_attn")
    m, cfg = _windowed_model(g)
    m = m.cuda().eval()
    x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
    with torch.no_grad():
        outs = [o.cpu() for o in m(x.cuda(), margin=margin.cuda())]
        again = [o.cpu() for o in m(x.cuda(), margin=margin.cuda())]          # (the second forward replays the graph)
    assert (m._engine.graph is not None) == (graph == "1")
    for got in (outs, again):
        worst = {}
        for n, o in zip(NAMES, got):
            ref = g["e2e_" + n]
            assert o.shape == ref.shape, n
            worst[n] = float((o - ref).abs().max())
            assert worst[n] <= 1e-3 * max(1.0, float(ref.abs().max())), f"{n}: max abs err {worst[n]}"
        assert worst["output"] <= 1e-3 and worst["rough"] <= 1e-3
    print("LOCALATTN|e2e|", worst)


def test_default_keys_are_bit_equal_to_no_keys():
    def run(cfg):
        m = OTPose(cfg)
        S.fill_synthetic_(m)
        m = m.cuda().eval()
        x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
        with torch.no_grad():
            outs = [o.clone() for o in m(x.cuda(), margin=margin.cuda())]
        return outs, len(m._engine.ops)
    cfg = tiny_cfg(8, (64, 96))
    cfg.MODEL.MHA_WIN_SIZE, cfg.MODEL.USE_REL_PE, cfg.MODEL.FLOW_MHA_WIN_SIZE = -1, False, -1
    (a, na), (b, nb) = run(tiny_cfg(8, (64, 96))), run(cfg)
    assert na == nb
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- training ---------------------------------------------------------------------------------------------------------------------
class _Holder(nn.Module):
    """What ``TrainGraph`` walks: a module tree with a ``cfg``."""

    def __init__(self, blk):
        super().__init__()
        self.b, self.cfg = blk, None


@pytest.mark.parametrize("stride", [1, 2])
def test_windowed_block_trains_like_fp64_autograd(stride):
    c, nh, t, win = 34, 2, 32, 9
    blk = M.TransformerBlock(c, nh, (stride, stride), 0.0, 0.0, 0.1, mha_win_size=win, use_rel_pe=True)
    rel = {"attn.rel_pe": seeded((1, 1, nh, win), 5, 0.5)}
    R.fill_windowed_(blk, 12, rel)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    x = seeded((2, c, t), 31)
    go = seeded((2, c, t // stride), 32)

    def reference(dtype):
        leaves = {k: v.detach().clone().to(dtype).requires_grad_() for k, v in sd.items()}
        xl = x.detach().clone().to(dtype).requires_grad_()
        y = R.transformer_block({"b." + k: v for k, v in leaves.items()}, "b", xl, nh, stride, win)
        y.backward(go.to(dtype))
        return y.detach(), xl.grad, {k: v.grad for k, v in leaves.items()}
    yr, gxr, gr = reference(D)
    yy, gxy, gy = reference(torch.float32)

    holder = _Holder(blk).cuda().train()
    holder.train_dropout = False
    graph = TR.TrainGraph(holder)
    xg = x.cuda().requires_grad_()
    with T.active_routes(graph.routes):
        y = graph.tblock("b", xg, nh, stride)
    y.backward(go.cuda())
    _check(f"tblock s{stride} y", y, yr, yy, 1e-4)
    _check(f"tblock s{stride} dx", xg.grad, gxr, gxy, 1e-4)
    for name, p in blk.named_parameters():
        assert p.grad is not None, name
        _check(f"tblock s{stride} d{name}", p.grad, gr[name], gy[name], 1e-4)
    assert "attn.rel_pe" in dict(blk.named_parameters())


def test_attention_dropout_is_not_implemented_in_training():
    blk = M.TransformerBlock(34, 2, (1, 1), attn_pdrop=0.1, mha_win_size=9)
    S.fill_synthetic_(blk, 12)
    graph = TR.TrainGraph(_Holder(blk).cuda().train())
    with pytest.raises(NotImplementedError), T.active_routes(graph.routes):
        graph.tblock("b", torch.zeros(1, 34, 32, device="cuda"), 2, 1)


def test_tiny_otpose_with_windows_trains(golden):
    g = golden("local_attn")

    def step():
        m, cfg = _windowed_model(g)
        m = m.cuda().train()
        m.train_dropout = False
        x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
        outs = TR.forward_train(m, x.cuda(), margin.cuda())
        b, j, h, w = outs[0].shape
        tgt, wt = S.synthetic_targets(b, (w, h), j, sigma=1.5, seed=77)
        loss = TR.criterion(outs, tgt.cuda(), wt.cuda())
        loss.backward()
        return loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if n.endswith("rel_pe")}
    loss, grads = step()
    assert bool(torch.isfinite(loss))
    assert len(grads) == 16 and all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in grads.values())
    loss2, grads2 = step()
    assert torch.equal(loss, loss2)
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n
