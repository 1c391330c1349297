"""RSN_ATTENTION / RSN_WEIGHT_VECTOR on the GPU (csrc/prm.hip): the two inference launches and the training Functions against the
float64 restatement of tests/prm_ref.py, the modules and a tiny OTPose with ``MODEL.PRM`` against the reference's own outputs
(tests/golden/prm.npz), the training graph, and the default model (same bits, same launch list).

Operator bound: ``tests/reductions_cases.bound`` - 4 x the error of the fp32 restatement on the CPU against float64 on the same
operands (at least 4 ulp of the largest reference magnitude, never above the tolerance of tests/test_gpu_train_ops.py).  Every
comparison prints a ``PRM|`` line with the error, the yardstick and the bound.

Tile constants of csrc/prm.hip that the shapes below are chosen from: an output tile is PRM_TH = 8 rows of PRM_TW = 32 pixels with a
4-pixel halo; the output channels pass through the LDS in chunks of 8 (C = 17, 20: 3 chunks, the last one partial) or 16 (C = 32:
2 chunks; C = 64: 4 chunks)."""
import functools

import pytest
import torch
from torch import nn

from otpose_amd import OTPose, hip, ops, tiny_cfg
from otpose_amd import modules as M
from otpose_amd import synthetic as S
from otpose_amd import train as TR
from otpose_amd import train_ops as T
from tests import prm_ref as R
from tests import reductions_cases as K
from tests.conftest import seeded
from tests.test_prm_host import CASES, PRM_BOTH, TRAIN_SHAPES, build_case, train_case, train_reference

pytestmark = pytest.mark.gpu
D = torch.float64
NAMES = ("output", "rough", "intersection", "prev_b", "context", "squeezed", "total_b")
PRM_TH, PRM_TW = 8, 32
# (N, C, H, W, scale of x).  (2, 17, 5, 7): the image is smaller than the 9x9 window, every tap meets the border; (1, 32, 13, 19): odd
# sizes, partial tiles; (3, 20, 19, 69): two whole tiles and a partial one in each direction (2 PRM_TH + 3, 2 PRM_TW + 5);
# (1, 64, 9, 8): the channel cap, four channel chunks; the first input once more, scaled until the gate logits saturate
FWD = [(2, 17, 5, 7, 1.0), (1, 32, 13, 19, 1.0), (3, 20, 2 * PRM_TH + 3, 2 * PRM_TW + 5, 1.0), (1, 64, 9, 8, 1.0), (2, 17, 5, 7, 40.0)]
FN_SHAPES = [(4, 17, 5, 7), (5, 20, 13, 19)]


def _check(name, got, ref, yard, cap=K.FWD_TOL, keep=None):
    """``keep``: a bool mask (broadcastable) of the elements compared."""
    got = got.detach().cpu().to(D)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if keep is not None:
        got, yard, ref = got * keep, yard * keep, ref * keep
    err, y = K.max_err(got, ref), K.max_err(yard, ref)
    b = K.bound(y, ref, cap)
    print(f"PRM|{name}|err {err:.3e}|yardstick {y:.3e}|ratio {err / y if y > 0 else float('nan'):.2f}|bound {b:.3e}|max|ref| "
          f"{float(ref.abs().max()):.3e}")
    assert err <= b, f"{name}: error {err:.3e} above bound {b:.3e} (fp32 yardstick {y:.3e})"


def _folded(sd, layers):
    out = []
    for p in layers:
        out += list(R.fold(sd, p))
    return out


@functools.lru_cache(maxsize=None)
def _fwd_case(n, c, h, w, scale):
    """fp32 operands of the two launches - f, the folded layers, the fp32 gate - and the module's state dict and input."""
    mod = R.fill_prm_(M.RSN_ATTENTION(c), 100 + c).eval()
    sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    x = seeded((n, c, h, w), 200 + c + h) * scale
    f = R.cbr(sd, "conv_bn_relu_prm_1", x)
    gate_l = _folded(sd, R.ATT_LAYERS[1:3])
    apply_l = _folded(sd, R.ATT_LAYERS[3:5])
    return mod, sd, x, f, gate_l, apply_l, R.prm_gate(f, *gate_l)


def _dbl(ts):
    return [t.double() for t in ts]


def _cuda(ts):
    return [t.cuda() for t in ts]


@pytest.mark.parametrize("shape", FWD)
def test_prm_gate_forward_vs_fp64(shape):
    _, _, _, f, gate_l, _, gate32 = _fwd_case(*shape)
    ref = R.prm_gate(f.double(), *_dbl(gate_l))
    got = ops.prm_gate(f.cuda(), *_cuda(gate_l))
    _check(f"gate {shape}", got, ref, gate32)
    assert torch.equal(got, ops.prm_gate(f.cuda(), *_cuda(gate_l)))


@pytest.mark.parametrize("shape", FWD)
def test_prm_apply_forward_vs_fp64(shape):
    _, sd, _, f, _, apply_l, gate32 = _fwd_case(*shape)
    ref = R.prm_apply(f.double(), gate32.double(), *_dbl(apply_l))
    yard = R.prm_apply(f, gate32, *apply_l)
    got = ops.prm_apply(f.cuda(), gate32.cuda(), *_cuda(apply_l))
    _check(f"apply {shape}", got, ref, yard)
    assert torch.equal(got, ops.prm_apply(f.cuda(), gate32.cuda(), *_cuda(apply_l)))


def test_saturated_case_reaches_the_flat_ends_of_the_sigmoid():
    """The scaled input of FWD[-1]: ReLU pre-activations in front of both sigmoids below -20 (the gate is sigmoid(0)) and logits
    above 20 (the gate is 1 to fp32)."""
    _, sd, x, *_ = _fwd_case(*FWD[-1])
    pre = {}
    R.rsn_attention({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, "", x.double(), pre=pre)
    for layer in ("conv_bn_relu_prm_2_2", "conv_bn_relu_prm_3_2"):
        assert float(pre[layer].max()) > 20.0 and float(pre[layer].min()) < -20.0, layer


@pytest.mark.parametrize("shape", FWD)
def test_rsn_attention_forward_vs_fp64(shape):
    mod, sd, x, *_ = _fwd_case(*shape)
    ref = R.rsn_attention({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, "", x.double())
    yard = R.rsn_attention(sd, "", x)
    _check(f"attention {shape}", ops.rsn_attention(x.cuda(), mod.cuda()), ref, yard)
    mod.cpu()


def test_zero_padding_applies_to_t_not_to_f():
    """The 9x9 pads t = ReLU(BN(1x1(f))) with zeros: a halo pixel outside the image is 0, not ReLU(shift) of a zero input.  With an
    all-zero f the output f (1 + ...) is zero whatever the halo holds, so that run can only show that nothing non-finite leaks
    out; the rule itself shows with a zero 1x1 weight and a positive folded shift - t is ReLU(shift) at every pixel of the image
    whatever f is - under f = 1: out = 1 + gate_c gate_s, whose border depends on what the halo holds."""
    n, c, h, w = 1, 17, 13, 19
    _, sd, _, _, _, apply_l, _ = _fwd_case(1, 17, 5, 7, 1.0)
    w31, sc31, sh31, w32, sc32, sh32 = apply_l
    sh31 = sh31.abs() + 0.5
    w32 = w32.abs()                                           # every tap pulls the same way: a filled halo cannot cancel
    gate = torch.full((n, c, 1, 1), 0.75)
    zero = torch.zeros(n, c, h, w)
    got0 = ops.prm_apply(zero.cuda(), gate.cuda(), *_cuda((w31, sc31, sh31, w32, sc32, sh32)))
    assert torch.equal(got0.cpu(), R.prm_apply(zero, gate, w31, sc31, sh31, w32, sc32, sh32)) and float(got0.abs().max()) == 0.0
    ones, w0 = torch.ones(n, c, h, w), torch.zeros_like(w31)
    args = (w0, sc31, sh31, w32, sc32, sh32)
    ref = R.prm_apply(ones.double(), gate.double(), *_dbl(args))
    yard = R.prm_apply(ones, gate, *args)
    got = ops.prm_apply(ones.cuda(), gate.cuda(), *_cuda(args))
    _check("padding", got, ref, yard)
    # what a halo of ReLU(shift) would give: the depthwise conv of a constant plane without a border
    t = torch.relu(sh31.double()).reshape(1, c, 1, 1)
    s = torch.relu(t * w32.double().reshape(c, -1).sum(1).reshape(1, c, 1, 1) * sc32.double().reshape(1, c, 1, 1)
                   + sh32.double().reshape(1, c, 1, 1))
    wrong = (1 + gate.double() * torch.sigmoid(s)).expand(n, c, h, w)
    border = torch.ones(h, w, dtype=torch.bool)
    border[4:-4, 4:-4] = False
    assert float((wrong - ref)[..., border].abs().max()) > 1e-3                   # the two rules differ on the border ...
    assert float((got.cpu().double() - ref)[..., border].abs().max()) < 1e-5      # ... and the kernel follows the restatement's
    assert float((wrong - ref)[..., ~border].abs().max()) < 1e-12


def test_prm_rejects_unsupported_arguments():
    L = hip.lib()
    assert L.otp_prm_supported(64, 9, 8) == 1 and L.otp_prm_supported(65, 9, 8) == 0 and L.otp_prm_supported(0, 9, 8) == 0
    f = torch.zeros(1, 65, 4, 4, device="cuda")
    w, v = torch.zeros(65, 65, device="cuda"), torch.zeros(65, device="cuda")
    with pytest.raises(ValueError):
        ops.prm_gate(f, w, v, v, w, v, v)
    with pytest.raises(ValueError):
        ops.prm_apply(f, torch.zeros(1, 65, device="cuda"), w, v, v, torch.zeros(65, 1, 9, 9, device="cuda"), v, v)
    f = torch.zeros(1, 8, 4, 4, device="cuda")
    w, v = torch.zeros(8, 8, device="cuda"), torch.zeros(8, device="cuda")
    with pytest.raises(ValueError):
        ops.prm_gate(f, w, v, v, torch.zeros(8, 7, device="cuda"), v, v)
    with pytest.raises(ValueError):
        ops.prm_apply(f, torch.zeros(2, 8, device="cuda"), w, v, v, torch.zeros(8, 1, 9, 9, device="cuda"), v, v)
    with pytest.raises(ValueError):
        ops.prm_apply(f, torch.zeros(1, 8, device="cuda"), w, v, v, torch.zeros(8, 1, 7, 7, device="cuda"), v, v)
    with pytest.raises(NotImplementedError):
        ops.prm_gate(f.cpu(), w.cpu(), v, v, w.cpu(), v, v)
    with pytest.raises(ValueError):
        T.dwconv2d(f, torch.zeros(8, 1, 7, 7, device="cuda"))
    p, bad = hip.ptr(f), hip.CONSTANTS["OTP_ERR_BAD_ARG"]
    assert L.otp_prm_apply(p, p, p, p, p, p, p, p, hip.ptr(w), 1, 65, 4, 4, hip.stream_of(f)) == bad
    assert L.otp_prm_apply(p, p, p, p, p, p, p, p, p, 1, 8, 4, 4, hip.stream_of(f)) == bad          # out aliases f
    assert L.otp_prm_gate(p, p, p, p, p, p, p, hip.ptr(w), 1, 65, 16, 0, hip.stream_of(f)) == bad
    assert L.otp_dwconv2d(p, p, None, hip.ptr(w), 1, 8, 4, 4, 7, 0, hip.stream_of(f)) == bad


# ---- modules against the reference's outputs -----------------------------------------------------------------------------------
def _close(name, got, ref, tol=5e-5):
    got = got.detach().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = float((got - ref).abs().max())
    print(f"PRM|golden {name}|err {err:.3e}|max|ref| {float(ref.abs().max()):.3e}")
    assert err <= tol * max(1.0, float(ref.abs().max())), err


@pytest.mark.parametrize("tag", sorted(CASES))
def test_modules_match_golden_through_the_engine_launches(golden, tag):
    from otpose_amd.engine import InferenceEngine
    from otpose_amd.ops import View
    g = golden("prm")
    mod = build_case(tag)
    x = g[tag + "_x"]
    eng = InferenceEngine.bare("cuda")
    xin = eng.new(*x.shape)
    xin.copy_(x)
    eng.inp = xin
    with torch.no_grad():
        if CASES[tag][0] == "RSN_ATTENTION":
            out = eng.rsn_attention(mod, View(xin)).t
            direct = ops.rsn_attention(x.cuda(), mod.cuda())
        else:
            out = eng.rsn_weight_vector(mod, View(xin))                          # (the residual flag of otp_prm_gate)
            direct = ops.rsn_weight_vector(x.cuda(), mod.cuda())
    assert len(eng.ops) == (3 if CASES[tag][0] == "RSN_ATTENTION" else 2)
    torch.cuda.synchronize()
    eng._launch_all()
    torch.cuda.synchronize()
    _close(tag + " engine", out, g[tag + "_y"])
    _close(tag + " ops", direct, g[tag + "_y"])


def _prm_cfg(dtype=None, size=(8, (64, 96))):
    cfg = tiny_cfg(*size) if dtype is None else tiny_cfg(*size, dtype=dtype)
    cfg.MODEL.PRM = PRM_BOTH
    return cfg


def _prm_model(dtype=None, size=(8, (64, 96))):
    cfg = _prm_cfg(dtype, size)
    return R.fill_prm_(OTPose(cfg), S.WEIGHT_SEED), cfg


def test_tiny_otpose_with_prm_matches_reference_graph_on_and_off(golden, monkeypatch):
    g = golden("prm")
    results = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("OTPOSE_HIP_GRAPH", graph)
        m, cfg = _prm_model()
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
        print("PRM|e2e graph", graph, "|", worst)
        results[graph] = outs
        del m
    for a, b in zip(results["1"], results["0"]):
        assert torch.equal(a, b)


def test_default_keys_are_bit_equal_to_no_keys_with_the_same_launch_list():
    def run(cfg, fill=S.fill_synthetic_):
        m = OTPose(cfg)
        fill(m)
        m = m.cuda().eval()
        x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
        with torch.no_grad():
            outs = [o.clone() for o in m(x.cuda(), margin=margin.cuda())]
        return outs, len(m._engine.ops)
    cfg = tiny_cfg(8, (64, 96))
    cfg.MODEL.PRM = ()
    (a, na), (b, nb) = run(tiny_cfg(8, (64, 96))), run(cfg)
    assert na == nb
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    _, n_prm = run(_prm_cfg(), lambda m: R.fill_prm_(m, S.WEIGHT_SEED))
    assert n_prm == na + 6                                   # conv, otp_prm_gate, otp_prm_apply behind each of the two chains


def test_fp16_engine_runs_the_prm_through_inheritance():
    """The fp16 engine overrides the backbone only and hands its tail fp32 tensors: it emits the same PRM launches (three per
    module more than without the key), its heat-maps are finite and a replay of its graph is bit-equal.  No bound is asserted
    here, as in the conv-embedding test."""
    from otpose_amd.engine_h16 import InferenceEngineH16
    n_ops = {}
    for prm in ((), PRM_BOTH):
        cfg = tiny_cfg(16, (128, 192), dtype="fp16")
        cfg.MODEL.PRM = prm
        m = R.fill_prm_(OTPose(cfg), S.WEIGHT_SEED).cuda().eval()
        x, margin = S.synthetic_clip(1, cfg.MODEL.IMAGE_SIZE)
        with torch.no_grad():
            outs = [o.clone() for o in m(x.cuda(), margin=margin.cuda())]
            again = m(x.cuda(), margin=margin.cuda())
        assert type(m._engine) is InferenceEngineH16
        assert all(bool(torch.isfinite(o).all()) for o in outs)
        for a_, b_ in zip(outs, again):
            assert torch.equal(a_, b_)
        n_ops[prm] = len(m._engine.ops)
    assert n_ops[PRM_BOTH] == n_ops[()] + 6


# ---- the training Functions ---------------------------------------------------------------------------------------------------------
def _fn_case(fn, leaves, go, run):
    """``run(*cuda leaves)`` against float64 and float32 autograd of ``fn``; twice, bit-equal."""
    ref, gref = R.autograd(fn, [t.double() for t in leaves], go.double())
    yard, gyard = R.autograd(fn, leaves, go)

    def once():
        ls = [t.cuda().requires_grad_() for t in leaves]
        out = run(*ls)
        out.backward(go.cuda())
        return out.detach(), [t.grad for t in ls]
    out, grads = once()
    out2, grads2 = once()
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    return (out, ref, yard), list(zip(grads, gref, gyard))


@pytest.mark.parametrize("shape", FN_SHAPES)
def test_spatial_mean_vs_fp64_and_deterministic(shape):
    x, go = seeded(shape, 300 + shape[1]) + 0.5, seeded(shape[:2] + (1, 1), 301 + shape[1])
    fwd, grads = _fn_case(R.spatial_mean, [x], go, T.spatial_mean)
    _check(f"spatial_mean {shape}", *fwd)
    _check(f"spatial_mean dx {shape}", *grads[0], cap=K.GRAD_TOL)


@pytest.mark.parametrize("shape", FN_SHAPES)
def test_prm_combine_vs_fp64_and_deterministic(shape):
    n, c = shape[:2]
    f, a, s = seeded(shape, 310 + c), seeded((n, c, 1, 1), 311 + c, 2.0), seeded(shape, 312 + c, 2.0)
    fwd, grads = _fn_case(R.prm_combine, [f, a, s], seeded(shape, 313 + c), T.prm_combine)
    _check(f"prm_combine {shape}", *fwd)
    for name, g in zip(("df", "da", "ds"), grads):
        _check(f"prm_combine {name} {shape}", *g, cap=K.GRAD_TOL)


@pytest.mark.parametrize("shape", FN_SHAPES)
def test_dwconv2d_vs_fp64_and_deterministic(shape):
    c = shape[1]
    x, w, b = seeded(shape, 320 + c), seeded((c, 1, 9, 9), 321 + c, 1.0 / 9), seeded((c,), 322 + c, 0.3)
    fwd, grads = _fn_case(R.dwconv2d, [x, w, b], seeded(shape, 323 + c), T.dwconv2d)
    _check(f"dwconv2d {shape}", *fwd)
    for name, g in zip(("dx", "dweight", "dbias"), grads):
        _check(f"dwconv2d {name} {shape}", *g, cap=K.GRAD_TOL)


# ---- the whole module in training mode -----------------------------------------------------------------------------------------------
class _Holder(nn.Module):
    """What ``TrainGraph`` walks: a module tree with a ``cfg``."""

    def __init__(self, blk):
        super().__init__()
        self.b, self.cfg = blk, None


def _train_graph(shape):
    sd, x, go = train_case(shape)
    mod = M.RSN_ATTENTION(shape[1])
    mod.load_state_dict(sd)
    holder = _Holder(mod).cuda().train()
    holder.train_dropout = False
    return mod, TR.TrainGraph(holder), x, go


@pytest.mark.parametrize("shape", TRAIN_SHAPES)
def test_rsn_attention_trains_like_fp64_autograd(shape):
    """Output, dx, every parameter gradient and the running statistics after one step against float64 autograd of the
    restatement in batch-statistics mode.  Pixels with a ReLU pre-activation within KINK_DELTA of zero in the float64 run are left
    out of the output and dx comparisons (tests/test_prm_host.py asserts their share and that no gate-vector value is one; with
    the seeds used there is none).

    Measured on the MI355X (error / yardstick E, bound 4 E): output 1.04 and 1.35, dx, all 40 parameter gradients and the running
    statistics at most 1.5.  The BatchNorm of the (N, C, 1, 1) gate vectors runs on the two-pass fp64 path of csrc/train.hip for
    channels with few values: with E[x^2] - mean^2 statistics four gradients were at 4.1 - 6.5 E."""
    ref, gxr, gr, stats_r, pre = train_reference(shape, D)
    yard, gxy, gy, stats_y, _ = train_reference(shape, torch.float32)
    keep = ~R.kink_pixels(pre, shape)
    left_out = 1.0 - float(keep.double().mean())
    print(f"PRM|train {shape}|pixels left out {left_out:.4f}")
    assert left_out <= R.KINK_CAP and all(share == 0.0 for share, vec in R.kink_report(pre).values() if vec)
    mod, graph, x, go = _train_graph(shape)
    before = {k: v.detach().clone() for k, v in mod.state_dict().items() if "running_" in k}
    xg = x.cuda().requires_grad_()
    with T.active_routes(graph.routes):
        out = graph.rsn_attention("b", xg)
    out.backward(go.cuda())
    failed = []
    checks = [("out", out, ref, yard, K.FWD_TOL, keep), ("dx", xg.grad, gxr, gxy, K.GRAD_TOL, keep)]
    P = dict(mod.named_parameters())
    assert sorted(P) == sorted(gr)
    checks += [("d" + k, P[k].grad, gr[k], gy[k], K.GRAD_TOL, None) for k in sorted(P)]
    after = mod.state_dict()
    for layer, (mean, var) in stats_r.items():
        for leaf, stat, stat_y in (("running_mean", mean, stats_y[layer][0]), ("running_var", var, stats_y[layer][1])):
            k = f"{layer}.bn.{leaf}"
            old = before[k].cpu()
            checks.append((k, after[k], 0.9 * old.double() + 0.1 * stat, 0.9 * old + 0.1 * stat_y, K.FWD_TOL, None))
    for name, got, r, y, cap, kp in checks:                  # every figure is printed before the first assertion speaks
        assert got is not None, name
        try:
            _check(f"train {shape} {name}", got, r, y, cap, kp)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)


def test_one_sample_in_training_mode_raises_before_any_launch():
    mod, graph, x, _ = _train_graph(TRAIN_SHAPES[0])
    before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        with T.active_routes(graph.routes):
            graph.rsn_attention("b", x[:1].cuda())
    assert all(torch.equal(v, before[k]) for k, v in mod.state_dict().items())     # no running statistic moved
    out = ops.rsn_attention(x[:1].cuda(), mod.eval())                             # eval mode takes N = 1
    assert out.shape == x[:1].shape and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tiny_otpose_with_prm_trains_deterministically(dtype):
    def steps():
        m, cfg = _prm_model()
        m = m.cuda().train()
        m.train_dtype = dtype
        m.train_dropout = False
        x, margin = S.synthetic_clip(2, cfg.MODEL.IMAGE_SIZE)
        losses = []
        for _ in range(2):
            m.zero_grad()
            outs = TR.forward_train(m, x.cuda(), margin.cuda())
            b, j, h, w = outs[0].shape
            tgt, wt = S.synthetic_targets(b, (w, h), j, sigma=1.5, seed=77)
            loss = TR.criterion(outs, tgt.cuda(), wt.cuda())
            loss.backward()
            losses.append(loss.detach().clone())
        return losses, {n: p.grad.clone() for n, p in m.named_parameters() if R.is_prm_key(n)}
    losses, grads = steps()
    assert all(bool(torch.isfinite(v)) for v in losses)
    assert len(grads) == 40 and all(bool(torch.isfinite(v).all()) for v in grads.values())
    assert any(float(v.abs().max()) > 0 for v in grads.values())
    losses2, grads2 = steps()
    assert all(torch.equal(a, b) for a, b in zip(losses, losses2))
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n
