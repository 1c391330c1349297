"""Conv embedding of ConvTransformer on the GPU (csrc/convembd.hip): the fused launch and its backward against the float64
restatement of tests/conv_embd_ref.py, the modules against the reference's own outputs (tests/golden/conv_embd.npz) through the
launches the inference engine emits, the tiny OTPose with ``MODEL.EMBD_LAYERS = 1`` (hipGraph on and off), and the training graph.

Operator bounds: with E the max-abs error of the fp32 restatement on the CPU against float64 on the same operands, the kernel
must be within 4 E - forward and every gradient.  A ReLU mask that flips between precisions changes a whole token's gradient
through the norm, so the backward tests give tokens in which any float64 pre-activation is within 1e-5 of zero a zero cotangent
(they then contribute to no gradient, in the reference, the yardstick and the kernel alike) and assert that fewer than 2 % of
the tokens are left out.  Every comparison prints a ``CONVEMBD|`` line with the error beside E.

The fixture's ConvTransformers are built with path_pdrop = 0, where the reference adds the residuals unscaled; the engine and the
training graph read the AffineDropPath scales, so the GPU cases build the same encoder with path_pdrop > 0 and scales of one."""
import functools

import pytest
import torch
from torch import nn

from otpose_amd import OTPose, hip, ops, tiny_cfg
from otpose_amd import modules as M
from otpose_amd import synthetic as S
from otpose_amd import train as TR
from otpose_amd import train_ops as T
from tests import conv_embd_ref as R
from tests import reductions_cases as K
from tests.conftest import seeded
from tests.test_conv_embd_host import CASES, build_case

pytestmark = pytest.mark.gpu
D = torch.float64
NAMES = ("output", "rough", "intersection", "prev_b", "context", "squeezed", "total_b")

# (B, Cin, Cout, H, W, ks, ln, bias, pe).  Channels: 8 / 17 / 40 / 100 / 136 / 204 reach the six instances of the kernel (Cout <= 16,
# 32, 64, 128, 192, 256) and input chunks of 4 and 8 channels with a remainder; grids: (12, 8) and (7, 5) sit inside one
# 128-pixel tile (the second with odd sizes), (3, 70) is one tile and a remainder with a row that straddles the tile edge,
# (16, 16) two whole tiles, (1, 1) a single pixel whose every tap but the centre is padding.
FWD = [
    (2, 17, 17, 12, 8, 3, True, False, True),
    (1, 136, 136, 12, 8, 3, True, False, True),
    (2, 136, 136, 7, 5, 5, True, False, False),
    (1, 24, 40, 7, 5, 5, False, True, False),
    (2, 24, 40, 3, 70, 3, True, True, True),
    (1, 204, 204, 3, 70, 1, True, False, False),
    (1, 204, 204, 12, 8, 3, False, True, True),
    (1, 17, 17, 3, 70, 5, False, False, False),
    (2, 136, 136, 3, 70, 1, False, True, True),
    (2, 24, 40, 12, 8, 1, True, False, True),
    (1, 136, 136, 16, 16, 3, True, False, True),
    (1, 8, 8, 7, 5, 3, True, False, False),
    (1, 40, 100, 7, 5, 3, True, False, True),
    (1, 3, 5, 1, 1, 5, True, False, False),
]
# the Function takes the kernel sizes the weight gradient is built for (1, 3)
BWD = [
    (2, 17, 17, 12, 8, 3, True, False),
    (1, 136, 136, 12, 8, 3, True, False),
    (2, 24, 40, 7, 5, 3, False, True),
    (2, 24, 40, 3, 70, 3, True, True),
    (1, 204, 204, 3, 70, 1, True, False),
    (1, 136, 136, 16, 16, 3, False, True),
    (1, 8, 8, 7, 5, 1, True, False),
]
MASK_EPS, MASK_CAP = 1e-5, 0.02


def _check(name, got, ref, yard):
    err, e = K.max_err(got, ref), K.max_err(yard, ref)
    print(f"CONVEMBD|{name}|err {err:.3e}|E {e:.3e}|ratio {err / e if e > 0 else float('nan'):.2f}|max|ref| "
          f"{float(ref.abs().max()):.3e}")
    assert err <= 4.0 * e, f"{name}: error {err:.3e} above 4 E = {4.0 * e:.3e}"


@functools.lru_cache(maxsize=None)
def _operands(b, cin, cout, h, w, ks, ln, bias, pe):
    seed = 1000 * cout + 10 * (h * w) + ks
    x = seeded((b, cin, h, w), seed)
    wt = seeded((cout, cin, ks, ks), seed + 1, (cin * ks * ks) ** -0.5)
    bs = seeded((cout,), seed + 2, 0.3) if bias else None
    gm = 1.0 + seeded((1, cout, 1), seed + 3, 0.2) if ln else None
    bt = seeded((1, cout, 1), seed + 4, 0.3) if ln else None
    p = seeded((cout, h * w), seed + 5) if pe else None
    return x, wt, bs, gm, bt, p


@functools.lru_cache(maxsize=None)
def _fwd_case(*shape):
    ops_ = _operands(*shape)
    dbl = [None if t is None else t.double() for t in ops_]
    return ops_, R.conv_embd(*dbl), R.conv_embd(*ops_)


def _cuda(ts):
    return [None if t is None else t.cuda() for t in ts]


@pytest.mark.parametrize("shape", FWD)
def test_conv_embd_forward_vs_fp64(shape):
    ops_, ref, yard = _fwd_case(*shape)
    out = ops.conv_embd(*_cuda(ops_))
    _check(f"fwd {shape}", out, ref, yard)


@functools.lru_cache(maxsize=None)
def _bwd_case(b, cin, cout, h, w, ks, ln, bias):
    """Operands, the cotangent (zero at the tokens next to a ReLU kink), and (output, gradients) in float64 and float32."""
    x, wt, bs, gm, bt, _ = _operands(b, cin, cout, h, w, ks, ln, bias, False)
    pre = R.pre_activation(x.double(), wt.double(), None if bs is None else bs.double(), None if gm is None else gm.double(),
                           None if bt is None else bt.double())
    near = (pre.abs() < MASK_EPS).any(dim=1, keepdim=True)                       # (B, 1, T)
    left_out = float(near.float().mean())
    go = seeded((b, cout, h * w), 77 + cout) * (~near)
    fn = lambda x_, w_, b_, g_, t_: R.conv_embd(x_, w_, b_, g_, t_)               # noqa: E731
    leaves = [x, wt, bs, gm, bt]
    ref = R.autograd(fn, [None if t is None else t.double() for t in leaves], go.double())
    yard = R.autograd(fn, leaves, go)
    return leaves, go, left_out, ref, yard


@pytest.mark.parametrize("shape", BWD)
def test_restatement_leaves_out_fewer_tokens_than_the_cap(shape):
    """CPU only in effect (no launch): the seeds of the backward cases keep the share of left-out tokens under the cap."""
    assert _bwd_case(*shape)[2] < MASK_CAP


@pytest.mark.parametrize("shape", BWD)
def test_conv_embd_function_backward_vs_fp64_and_deterministic(shape):
    leaves, go, left_out, (ref, gref), (yard, gyard) = _bwd_case(*shape)
    assert left_out < MASK_CAP, left_out

    def run():
        ls = [None if t is None else t.cuda().requires_grad_() for t in leaves]
        out = T.conv_embd(*ls)
        out.backward(go.cuda())
        return out.detach(), [None if t is None else t.grad for t in ls]
    out, grads = run()
    _check(f"train fwd {shape}", out, ref, yard)
    for name, g, r, y in zip(("dx", "dweight", "dbias", "dgamma", "dbeta"), grads, gref, gyard):
        if r is not None:
            assert g is not None and g.shape == r.shape, name
            _check(f"{name} {shape}", g, r, y)
    out2, grads2 = run()
    assert torch.equal(out, out2)
    for g, g2 in zip(grads, grads2):
        assert g is None or torch.equal(g, g2)


@pytest.mark.parametrize("shape", [BWD[1], BWD[3], BWD[2]])
def test_backward_pre_grad_z_vs_fp64_and_deterministic(shape):
    """``otp_conv_embd_backward_pre`` by itself: z from the forward launch, then grad_z, grad_gamma, grad_beta."""
    b, cin, cout, h, w, ks, ln, bias = shape
    (x, wt, bs, gm, bt), go, left_out, _, _ = _bwd_case(*shape)
    assert left_out < MASK_CAP
    t = h * w

    def tail(z_, b_, g_, t_):
        v = z_ if b_ is None else z_ + b_.reshape(1, cout, 1)
        if g_ is not None:
            res = v - v.mean(dim=1, keepdim=True)
            v = res / torch.sqrt((res ** 2).mean(dim=1, keepdim=True) + 1e-5) * g_ + t_
        return torch.relu(v)
    z64 = torch.nn.functional.conv2d(x.double(), wt.double(), None, 1, ks // 2).flatten(2)
    z32 = torch.nn.functional.conv2d(x, wt, None, 1, ks // 2).flatten(2)
    _, gref = R.autograd(tail, [z64] + [None if p is None else p.double() for p in (bs, gm, bt)], go.double())
    _, gyard = R.autograd(tail, [z32, bs, gm, bt], go)

    L = hip.lib()
    xc, goc = x.cuda(), go.cuda()
    bsc, gmc, btc, _ = ops.conv_embd_params(x.shape, wt, bs, gm, bt, None, xc.device)
    out, z = torch.empty(b, cout, t, device="cuda"), torch.empty(b, cout, t, device="cuda")
    hip.check(L.otp_conv_embd(*ops.conv_embd_args(xc, ops.pack_conv_embd_weight(wt.cuda()), bsc, gmc, btc, None, out, z, cout, ks,
                                                  1e-5), hip.stream_of(xc)), "otp_conv_embd")
    _check(f"z {shape}", z, z64, z32)

    def run():
        gz = torch.empty_like(z)
        gg = torch.empty(cout, device="cuda") if ln else None
        gb = torch.empty(cout, device="cuda") if ln else None
        n = L.otp_conv_embd_backward_pre_workspace(b, cout, t)
        ws = torch.empty(n // 4, device="cuda") if ln else None
        hip.check(L.otp_conv_embd_backward_pre(hip.ptr(z), hip.ptr(bsc), hip.ptr(gmc), hip.ptr(btc), hip.ptr(goc), hip.ptr(gz),
                                               hip.ptr(gg), hip.ptr(gb), hip.ptr(ws), n if ln else 0, b, cout, t, 1e-5,
                                               hip.stream_of(z)), "otp_conv_embd_backward_pre")
        return gz, gg, gb
    gz, gg, gb = run()
    _check(f"dz {shape}", gz, gref[0], gyard[0])
    if ln:
        _check(f"dgamma(pre) {shape}", gg.reshape(1, cout, 1), gref[2], gyard[2])
        _check(f"dbeta(pre) {shape}", gb.reshape(1, cout, 1), gref[3], gyard[3])
    for a, c in zip((gz, gg, gb), run()):
        assert a is None or torch.equal(a, c)


def test_conv_embd_rejects_unsupported_arguments():
    L = hip.lib()
    x = torch.zeros(1, 24, 7, 5, device="cuda")
    g, b = torch.ones(1, 40, 1, device="cuda"), torch.zeros(1, 40, 1, device="cuda")
    for wshape in [(40, 24, 2, 2), (257, 24, 3, 3), (40, 25, 3, 3), (40, 24, 7, 7)]:
        w = torch.zeros(*wshape, device="cuda")
        gg = torch.ones(1, wshape[0], 1, device="cuda")
        with pytest.raises(ValueError):
            ops.conv_embd(x, w, None, gg, torch.zeros_like(gg))
        assert L.otp_conv_embd_supported(1, wshape[1], 7, 5, wshape[0], wshape[2]) == (1 if wshape == (40, 25, 3, 3) else 0)
    w = torch.zeros(40, 24, 3, 3, device="cuda")
    with pytest.raises(ValueError):
        ops.conv_embd(x, w, None, g, None)
    with pytest.raises(ValueError):
        ops.conv_embd(x, w, torch.zeros(39, device="cuda"), g, b)
    with pytest.raises(ValueError):
        ops.conv_embd(x, w, None, g, b, pe=torch.zeros(40, 36, device="cuda"))
    with pytest.raises(ValueError, match="training"):
        T.conv_embd(x, torch.zeros(40, 24, 5, 5, device="cuda"), None, g, b)
    with pytest.raises(NotImplementedError):
        ops.conv_embd(x.cpu(), w.cpu(), None, g.cpu(), b.cpu())
    p = hip.ptr(x)
    bad = hip.CONSTANTS["OTP_ERR_BAD_ARG"]
    assert L.otp_conv_embd(p, p, None, None, None, None, p, None, 1, 24, 7, 5, 40, 2, 1e-5, hip.stream_of(x)) == bad
    assert L.otp_conv_embd(p, p, None, None, None, None, p, None, 1, 24, 7, 5, 257, 3, 1e-5, hip.stream_of(x)) == bad


# ---- modules against the reference's outputs -----------------------------------------------------------------------------------
def _close(got, ref, tol=5e-5):
    got = got.detach().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = float((got - ref).abs().max())
    print(f"CONVEMBD|golden|err {err:.3e}|max|ref| {float(ref.abs().max()):.3e}")
    assert err <= tol * max(1.0, float(ref.abs().max())), err


def _runnable(tag):
    """The fixture's encoder ``tag`` as one the engine and the training graph take: path_pdrop > 0 with every scale one."""
    src, n_head, arch = build_case(tag)
    args, kw, _, _ = CASES[tag]
    ct = M.ConvTransformer(*args, **kw, path_pdrop=0.1)
    missing = ct.load_state_dict(src.state_dict(), strict=False)
    assert not missing.unexpected_keys and all(k.endswith(".scale") for k in missing.missing_keys)
    with torch.no_grad():
        for k, v in ct.state_dict().items():
            if k.endswith(".scale"):
                v.fill_(1.0)
    return ct.eval(), n_head, arch


@pytest.mark.parametrize("tag", sorted(CASES))
def test_conv_transformer_with_embedding_matches_golden(golden, tag):
    from otpose_amd.engine import InferenceEngine
    g = golden("conv_embd")
    ct, n_head, arch = _runnable(tag)
    x4 = g[tag + "_x"]
    b, cin, h, w = x4.shape
    c, levels = ct.n_embd, arch[2] + 1
    eng = InferenceEngine.bare("cuda")
    xin = eng.new(b, cin, h * w)
    xin.copy_(x4.reshape(b, cin, h * w))
    eng.inp = xin
    stacked = eng.new(b, levels * c, h * w)
    with torch.no_grad():
        assert float(eng.encoder_pe(ct, h * w).abs().max()) == 0.0              # the table is added behind the last layer
        eng.conv_transformer(ct, xin, stacked)
    assert len(eng.ops) > arch[0]
    torch.cuda.synchronize()
    eng._launch_all()
    torch.cuda.synchronize()
    for i in range(levels):
        _close(stacked[:, i * c:(i + 1) * c], g[f"{tag}_y{i}"].reshape(b, c, h * w))


def _embd_cfg(dtype=None):
    cfg = tiny_cfg(8, (64, 96)) if dtype is None else tiny_cfg(8, (64, 96), dtype=dtype)
    cfg.MODEL.EMBD_LAYERS = 1
    return cfg


def _embd_model(dtype=None):
    cfg = _embd_cfg(dtype)
    return R.fill_embd_(OTPose(cfg), S.WEIGHT_SEED), cfg


def test_tiny_otpose_with_embedding_matches_reference_graph_on_and_off(golden, monkeypatch):
    g = golden("conv_embd")
    results = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("OTPOSE_HIP_GRAPH", graph)
        m, cfg = _embd_model()
        m = m.cuda().eval()
        x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
        with torch.no_grad():
            outs = [o.cpu() for o in m(x.cuda(), margin=margin.cuda())]
            again = [o.cpu() for o in m(x.cuda(), margin=margin.cuda())]       # (the second forward replays the graph)
        assert (m._engine.graph is not None) == (graph == "1")
        for got in (outs, again):
            worst = {}
            for n, o in zip(NAMES, got):
                ref = g["e2e_" + n]
                assert o.shape == ref.shape, n
                worst[n] = float((o - ref).abs().max())
                assert worst[n] <= 1e-3 * max(1.0, float(ref.abs().max())), f"{n}: max abs err {worst[n]}"
            assert worst["output"] <= 1e-3 and worst["rough"] <= 1e-3
        print("CONVEMBD|e2e graph", graph, "|", worst)
        results[graph] = outs
        del m
    for a, b in zip(results["1"], results["0"]):
        assert torch.equal(a, b)


def test_default_keys_are_bit_equal_to_no_keys_with_the_same_launch_list():
    def run(cfg):
        m = OTPose(cfg)
        S.fill_synthetic_(m)
        m = m.cuda().eval()
        x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
        with torch.no_grad():
            outs = [o.clone() for o in m(x.cuda(), margin=margin.cuda())]
        return outs, len(m._engine.ops)
    cfg = tiny_cfg(8, (64, 96))
    cfg.MODEL.EMBD_LAYERS, cfg.MODEL.FLOW_EMBD_LAYERS, cfg.MODEL.EMBD_KS, cfg.MODEL.EMBD_WITH_LN = 0, 0, 3, True
    (a, na), (b, nb) = run(tiny_cfg(8, (64, 96))), run(cfg)
    assert na == nb
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    m, ecfg = _embd_model()
    m = m.cuda().eval()
    x, margin = S.synthetic_clip(1, ecfg.MODEL.IMAGE_SIZE)
    with torch.no_grad():
        m(x.cuda(), margin=margin.cuda())
    assert len(m._engine.ops) == na + 2                                          # one launch per encoder with an embedding layer


def test_fp16_engine_runs_the_embedding_through_inheritance():
    """The fp16 engine overrides the backbone only and hands its encoders the same fp32 (B, C, T) tensors: it emits the same
    otp_conv_embd launches (one per embedding layer more than without the keys), its heat-maps are finite and a replay of its
    graph is bit-equal.  No bound against the fp32 engine is asserted: the LayerNorm of the 17-channel flow embedding
    re-normalises background tokens whose variance is near eps, which amplifies the backbone's fp16 rounding by a factor no
    reasoning bounds (measured: `context` 9.8e-3 of its range, against 8e-3 for the model without the embedding)."""
    from otpose_amd.engine_h16 import InferenceEngineH16
    n_ops = {}
    for layers in (0, 1):
        cfg = tiny_cfg(16, (128, 192), dtype="fp16")
        cfg.MODEL.EMBD_LAYERS, cfg.MODEL.FLOW_EMBD_LAYERS = layers, layers
        m = R.fill_embd_(OTPose(cfg), S.WEIGHT_SEED).cuda().eval()
        x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
        with torch.no_grad():
            outs = [o.clone() for o in m(x.cuda(), margin=margin.cuda())]
            again = m(x.cuda(), margin=margin.cuda())
        assert type(m._engine) is InferenceEngineH16
        assert all(bool(torch.isfinite(o).all()) for o in outs)
        for a_, b_ in zip(outs, again):
            assert torch.equal(a_, b_)
        n_ops[layers] = len(m._engine.ops)
    assert n_ops[1] == n_ops[0] + 3


# ---- training ---------------------------------------------------------------------------------------------------------------------
class _Holder(nn.Module):
    """What ``TrainGraph`` walks: a module tree with a ``cfg``."""

    def __init__(self, blk):
        super().__init__()
        self.b, self.cfg = blk, None


def _train_case(with_ln, c=34):
    c_in, nh, h, w = 20, 2, 8, 4
    ct = M.ConvTransformer(c_in, c, nh, 3, h * w, (1, 1, 1), h=h, path_pdrop=0.1, with_ln=with_ln)
    R.fill_embd_(ct, 21)
    x = seeded((2, c_in, h, w), 41)
    gos = [seeded((2, c, h * w), 42), seeded((2, c, h * w), 43)]
    return ct, nh, x, gos


def _check_cap(name, got, ref, yard, cap=1e-4):
    """The bound of the local-attention training test: tests/reductions_cases.bound."""
    err, y = K.max_err(got, ref), K.max_err(yard, ref)
    b = K.bound(y, ref, cap)
    print(f"CONVEMBD|{name}|err {err:.3e}|yardstick {y:.3e}|bound {b:.3e}|max|ref| {float(ref.abs().max()):.3e}")
    assert err <= b, f"{name}: error {err:.3e} above bound {b:.3e} (fp32 yardstick {y:.3e})"


@pytest.mark.parametrize("with_ln", [True, False])
def test_conv_transformer_with_embedding_trains_like_fp64_autograd(with_ln, monkeypatch):
    """Loss, input gradient and the gradients of the embedding parameters of a whole encoder against float64 autograd of the
    restatement, under the bound of the local-attention training test (4 x the fp32 yardstick, tests/reductions_cases.bound).

    The blocks behind the embedding run on their exact-fp32 routes here (``OTPOSE_CONV_MATH=f32`` for the graph's routes and
    ``otp_chan_attn_set_split(0)``, the switch tests/test_gpu_train_ops.py uses): the gradient that reaches the embedding has
    passed two blocks, and with their default split products (bfloat16 pieces for gradient operands, 2^-17 per operand) it
    arrives with 6 to 17 times the yardstick's error, which this test would then pin on the embedding.  Measured on the MI355X,
    error / yardstick with the default routes and with the exact ones: dx 5.6 / 1.4, d embd.0.weight 6.1 / 0.8, d embd_norm.0.weight
    8.3 / 0.8, d embd_norm.0.bias 8.6 / 0.7 (with_ln); dx 7.6 / 0.9, d embd.0.weight 9.2 / 1.0, d embd.0.bias 17.1 / 1.1 (without);
    the loss 1.0 / 1.1 and 0.1 / 1.0."""
    import os
    from otpose_amd import hip
    previous = 0 if os.environ.get("OTPOSE_CONV_MATH", "x3") == "f32" else 1      # what otpose_amd/hip.py set at load
    monkeypatch.setenv("OTPOSE_CONV_MATH", "f32")
    hip.lib().otp_chan_attn_set_split(0)
    try:
        _train_vs_fp64(with_ln)
    finally:
        hip.lib().otp_chan_attn_set_split(previous)


def _train_vs_fp64(with_ln):
    ct, nh, x, gos = _train_case(with_ln)
    sd = {k: v.detach().clone() for k, v in ct.state_dict().items()}
    embd = [k for k, _ in ct.named_parameters() if R.is_embd_key(k)]
    assert len(embd) == (3 if with_ln else 2)

    def reference(dtype):
        leaves = {k: v.detach().clone().to(dtype).requires_grad_() for k, v in sd.items() if v.is_floating_point()}
        xl = x.detach().clone().to(dtype).requires_grad_()
        outs = R.conv_transformer({"b." + k: v for k, v in leaves.items()}, "b", xl, nh, (1, 1, 1))
        loss = sum((o * go.to(dtype)).sum() for o, go in zip(outs, gos)) / x.numel()
        loss.backward()
        return loss.detach(), xl.grad, {k: leaves[k].grad for k in embd}
    lr, gxr, gr = reference(D)
    ly, gxy, gy = reference(torch.float32)

    holder = _Holder(ct).cuda().train()
    holder.train_dropout = False
    graph = TR.TrainGraph(holder)
    xg = x.cuda().requires_grad_()
    with T.active_routes(graph.routes):
        outs = graph.conv_transformer("b", xg, nh, (1, 1, 1))
    loss = sum((o * go.cuda()).sum() for o, go in zip(outs, gos)) / x.numel()
    loss.backward()
    P = dict(ct.named_parameters())
    checks = [("loss", loss.reshape(1), lr.reshape(1), ly.reshape(1)), ("dx", xg.grad, gxr, gxy)]
    checks += [("d" + k, P[k].grad, gr[k], gy[k]) for k in embd]
    failed = []
    for name, got, ref, yard in checks:                      # every figure is printed before the first assertion speaks
        assert got is not None, name
        try:
            _check_cap(f"train ln={with_ln} {name}", got, ref, yard)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)


def test_bf16_training_graph_runs_the_embedding_through_inheritance():
    """``TrainGraphBF16`` hands its encoders the same fp32 tensors: the embedding node is the fp32 one.  Its output and gradients
    agree with the fp32 graph's to the rounding of the bfloat16 layers behind it (8 significand bits, a handful of layers: a few
    per cent of the largest value) and point the same way."""
    ct, nh, x, gos = _train_case(True, c=40)               # C % 8 == 0, T % 32 == 0: the stem's MLP runs in bfloat16
    res = {}
    for name, cls in (("f32", TR.TrainGraph), ("bf16", TR.TrainGraphBF16)):
        ct.zero_grad()
        holder = _Holder(ct).cuda().train()
        holder.train_dropout = False
        graph = cls(holder)
        xg = x.cuda().requires_grad_()
        with T.active_routes(graph.routes):
            outs = graph.conv_transformer("b", xg, nh, (1, 1, 1))
        sum((o.float() * go.cuda()).sum() for o, go in zip(outs, gos)).backward()
        res[name] = ([o.detach().float() for o in outs], ct.embd[0].weight.grad.clone(), xg.grad.clone())
    for a, b in zip(res["f32"][0], res["bf16"][0]):
        assert float((a - b).abs().max()) <= 5e-2 * float(a.abs().max())
    for a, b in zip(res["f32"][1:], res["bf16"][1:]):
        assert bool(torch.isfinite(b).all())
        assert float(torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0)) > 0.99


def test_tiny_otpose_with_embedding_trains_deterministically():
    def step():
        m, cfg = _embd_model()
        m = m.cuda().train()
        m.train_dropout = False
        x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
        outs = TR.forward_train(m, x.cuda(), margin.cuda())
        b, j, h, w = outs[0].shape
        tgt, wt = S.synthetic_targets(b, (w, h), j, sigma=1.5, seed=77)
        loss = TR.criterion(outs, tgt.cuda(), wt.cuda())
        loss.backward()
        return loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if R.is_embd_key(n)}
    loss, grads = step()
    assert bool(torch.isfinite(loss))
    assert len(grads) == 6 and all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in grads.values())
    loss2, grads2 = step()
    assert torch.equal(loss, loss2)
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n
