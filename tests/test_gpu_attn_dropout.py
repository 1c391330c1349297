"""Attention-probability dropout on the GPU: the mask writer against the numpy restatement (bit-equal), the three attentions with
dropout against float64 restatements that take the SAME mask (tests/attn_dropout_ref.py), so dropout adds no error of its own and
the bounds are the ones of the undropped kernels' tests:

  token, local   ``reductions_cases.bound(yardstick, ref, cap)`` - four times the error of the fp32 restatement on the same
                 operands and mask, at least 4 ulp of the reference's maximum, never above cap * max(1, max|ref|); cap 3e-5
                 forward, 1e-4 gradients (tests/test_gpu_token_attn.py, tests/test_gpu_local_attn.py)
  channel        ``encoder_bwd_cases.attn_bound``: max(4 x yardstick, 2e-4 of the maximum), capped at 2e-4 of max(1, max|ref|)
                 (tests/test_gpu_encoder_bwd.py::test_chan_attn_backward_vs_fp64: split-product kernels)

and the tiny OTPose with the three ``cfg`` keys through one training step.  Every comparison prints an ``ATTNDROP|`` line."""
import functools
import math

import numpy as np
import pytest
import torch

from otpose_amd import attn_dropout as AD
from otpose_amd import token_attn as TA
from otpose_amd import train_ops as T
from tests import attn_dropout_ref as A
from tests import encoder_bwd_cases as C
from tests import reductions_cases as K
from tests.conftest import seeded

pytestmark = pytest.mark.gpu
D = torch.float64
TILE = 64
SEED = 0xC0FFEE0123456789
ROW_SEED = 0x123456789ABCDEF          # p = 0.5, (1, 5, 5): one row with every entry dropped (tests/test_attn_dropout_host.py)
RATES = [0.1, 0.5]


def _check(name, got, ref, yard, cap, bound=None):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: inf or NaN"
    err, y = K.max_err(got, ref), K.max_err(yard, ref)
    b = bound(y, ref) if bound else K.bound(y, ref, cap)
    print(f"ATTNDROP|{name}|err {err:.3e}|yardstick {y:.3e}|bound {b:.3e}|max|ref| {float(ref.abs().max()):.3e}")
    assert err <= b, f"{name}: error {err:.3e} above bound {b:.3e} (fp32 yardstick {y:.3e})"


# ---- the mask ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("shape", [(3, 5, 5), (2, 70, 131), (1, 1030, 1030), (4, 68, 68), (16, 64, 33)])
def test_keep_mask_is_bit_equal_to_the_restatement(shape, p):
    for seed in (SEED, ROW_SEED, 0):
        got = AD.keep_mask(seed, *shape, p, "cuda")
        assert got.dtype == torch.uint8 and tuple(got.shape) == shape
        assert np.array_equal(got.cpu().numpy().astype(bool), A.keep(seed, *shape, p)), (shape, p, hex(seed))


def test_keep_mask_without_dropout_keeps_everything():
    assert bool((AD.keep_mask(SEED, 2, 9, 7, 0.0, "cuda") == 1).all())


# ---- token attention -------------------------------------------------------------------------------------------------------------
# (B, C, n_head, T)
TOKEN_SHAPES = [(1, 5, 1, 5), (2, 17, 1, 35), (2, 136, 2, 108), (1, 204, 2, 333), (1, 64, 2, 1030)]
TOKEN_MASKS = ["none", "scattered", "first_tile"]


def make_mask(kind, b, t, seed):
    """The key-padding masks of tests/test_gpu_token_attn.py, restated: (B, T) bool, True = padding, or None; a shape too short
    for the tile case takes the scattered mask."""
    if kind == "none":
        return None
    mask = torch.zeros(b, t, dtype=torch.bool)
    if kind == "first_tile" and t > TILE:
        mask[:, :TILE] = True
    else:
        g = torch.Generator().manual_seed(seed)
        mask = torch.rand(b, t, generator=g) < 0.3
        mask[:, int(torch.randint(t, (1,), generator=g))] = False
    assert bool((~mask).any(dim=1).all()), "every sample keeps a live key"
    return mask


def _dev(x):
    return None if x is None else x.cuda()


@functools.lru_cache(maxsize=None)
def _token_case(b, c, nh, t, kind, p, seed):
    """Operands, the float64 reference and the fp32 yardstick (forward and gradients) under the restated mask, computed once."""
    s0 = 11 * t + c + nh
    q, k, v, go = (seeded((b, c, t), s0 + i) for i in range(4))
    mask = make_mask(kind, b, t, s0 + 5)
    scale = 1.0 / math.sqrt(c // nh)
    m = A.factors(seed, b * nh, t, t, p)
    fn = lambda q_, k_, v_: A.token_attn(q_, k_, v_, nh, scale, m, mask)          # noqa: E731
    ref = A.autograd(fn, [q.double(), k.double(), v.double()], go.double())
    yard = A.autograd(fn, [q, k, v], go)
    return (q, k, v, go, mask, scale), ref, yard


def _token_run(case, nh, p, seed):
    q, k, v, go, mask, scale = case
    leaves = [x.cuda().requires_grad_() for x in (q, k, v)]
    out = TA.token_attn(*leaves, nh, scale, _dev(mask), dropout_p=p, seed=seed)
    out.backward(go.cuda())
    return out.detach(), [x.grad for x in leaves]


@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("kind", TOKEN_MASKS)
@pytest.mark.parametrize("shape", TOKEN_SHAPES)
def test_token_attn_dropout_vs_fp64(shape, kind, p):
    case, (ref, gref), (yard, gyard) = _token_case(*shape, kind, p, SEED + shape[3])
    q, k, v, _, mask, scale = case
    out, grads = _token_run(case, shape[2], p, SEED + shape[3])
    _check(f"token fwd {shape} mask={kind} p={p}", out, ref, yard, 3e-5)
    for name, g, r, y in zip(("dq", "dk", "dv"), grads, gref, gyard):
        _check(f"token {name} {shape} mask={kind} p={p}", g, r, y, 1e-4)
    if mask is not None:
        dead = mask.cuda()[:, None, :].expand_as(grads[1])
        assert bool((grads[1][dead] == 0).all()) and bool((grads[2][dead] == 0).all()), "masked keys receive exactly zero dk / dv"
    with torch.no_grad():                                           # dropout under no_grad: forward only, the same mask
        assert torch.equal(TA.token_attn(q.cuda(), k.cuda(), v.cuda(), shape[2], scale, _dev(mask), dropout_p=p,
                                         seed=SEED + shape[3]), out)


def test_token_attn_dropped_row_is_exactly_zero():
    shape = (1, 5, 1, 5)
    case, (ref, gref), (yard, gyard) = _token_case(*shape, "none", 0.5, ROW_SEED)
    keep = A.keep(ROW_SEED, 1, 5, 5, 0.5)
    dead = [i for i in range(5) if not keep[0, i].any()]
    assert len(dead) == 1
    out, grads = _token_run(case, 1, 0.5, ROW_SEED)
    assert bool((out[0, :, dead[0]] == 0).all()), out
    assert float(out.abs().sum()) > 0
    _check("token dropped row fwd", out, ref, yard, 3e-5)
    for name, g, r, y in zip(("dq", "dk", "dv"), grads, gref, gyard):
        assert bool(torch.isfinite(g).all()), name
        _check(f"token dropped row {name}", g, r, y, 1e-4)
    assert bool((grads[0][0, :, dead[0]] == 0).all()), "a query whose row is dropped gets no gradient"


@pytest.mark.parametrize("shape", [(2, 17, 1, 35), (1, 64, 2, 1030)])
def test_token_attn_dropout_repeats_with_the_seed_and_zero_rate_is_the_plain_call(shape):
    case, _, _ = _token_case(*shape, "scattered", 0.5, SEED)
    q, k, v, go, mask, scale = case
    out, grads = _token_run(case, shape[2], 0.5, SEED)
    out2, grads2 = _token_run(case, shape[2], 0.5, SEED)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    out3, grads3 = _token_run(case, shape[2], 0.5, SEED + 1)
    assert not torch.equal(out, out3) and not torch.equal(grads[2], grads3[2])
    # a zero rate with a seed: the existing path, bit for bit
    plain_out, plain_grads = _token_run(case, shape[2], 0.0, None)
    zero_out, zero_grads = _token_run(case, shape[2], 0.0, SEED)
    assert torch.equal(plain_out, zero_out) and all(torch.equal(a, b) for a, b in zip(plain_grads, zero_grads))
    leaves = [x.cuda().requires_grad_() for x in (q, k, v)]
    old = TA.token_attn(*leaves, shape[2], scale, _dev(mask))
    old.backward(go.cuda())
    assert torch.equal(old.detach(), plain_out) and all(torch.equal(x.grad, g) for x, g in zip(leaves, plain_grads))
    assert not torch.equal(out, plain_out)


def test_token_attn_draws_its_seed_from_the_cuda_generator():
    case, _, _ = _token_case(2, 17, 1, 35, "none", 0.5, SEED)
    q, k, v, _, _, scale = case
    run = lambda: TA.token_attn(q.cuda(), k.cuda(), v.cuda(), 1, scale, dropout_p=0.5)      # noqa: E731
    with torch.no_grad():
        torch.manual_seed(3)
        a, b = run(), run()
        torch.manual_seed(3)
        a2 = run()
        off = torch.cuda.default_generators[torch.cuda.current_device()].get_offset()
        TA.token_attn(q.cuda(), k.cuda(), v.cuda(), 1, scale, dropout_p=0.0)                # no dropout: nothing is drawn
        assert torch.cuda.default_generators[torch.cuda.current_device()].get_offset() == off
    assert torch.equal(a, a2) and not torch.equal(a, b)


# ---- local-window attention --------------------------------------------------------------------------------------------------------
# (B, C, n_head, T, window): the smallest shapes of tests/test_gpu_local_attn.py with windows 5 and 33, two heads each
LOCAL_SHAPES = [(2, 34, 2, 4, 5), (2, 204, 2, 1056, 33)]


@functools.lru_cache(maxsize=None)
def _local_case(b, c, nh, t, win, rel, p):
    s0 = 7 * t + win + c
    q, k, v, go = (seeded((b, c, t), s0 + i) for i in range(4))
    rp = seeded((1, 1, nh, win), s0 + 9, 0.5) if rel else None
    scale = 1.0 / math.sqrt(c // nh)
    m = A.factors(SEED + win, b * nh, t, win, p)
    fn = lambda q_, k_, v_, r_: A.local_attn(q_, k_, v_, nh, win, scale, m, r_)          # noqa: E731
    ref = A.autograd(fn, [None if x is None else x.double() for x in (q, k, v, rp)], go.double())
    yard = A.autograd(fn, [q, k, v, rp], go)
    return (q, k, v, rp, go, scale), ref, yard


@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("rel", [False, True])
@pytest.mark.parametrize("shape", LOCAL_SHAPES)
def test_local_attn_dropout_vs_fp64(shape, rel, p):
    b, c, nh, t, win = shape
    (q, k, v, rp, go, scale), (ref, gref), (yard, gyard) = _local_case(*shape, rel, p)

    def run(seed):
        leaves = [x.cuda().requires_grad_() for x in (q, k, v)] + [None if rp is None else rp.cuda().requires_grad_()]
        out = T.local_attn(leaves[0], leaves[1], leaves[2], nh, win, scale, leaves[3], dropout_p=p, seed=seed)
        out.backward(go.cuda())
        return out.detach(), [None if x is None else x.grad for x in leaves]
    out, grads = run(SEED + win)
    _check(f"local fwd {shape} rel={rel} p={p}", out, ref, yard, 3e-5)
    for name, g, r, y in zip(("dq", "dk", "dv", "drel_pe"), grads, gref, gyard):
        if r is not None:
            _check(f"local {name} {shape} rel={rel} p={p}", g, r, y, 1e-4)
    out2, grads2 = run(SEED + win)
    assert torch.equal(out, out2) and all(g is None or torch.equal(g, g2) for g, g2 in zip(grads, grads2))
    assert not torch.equal(out, run(SEED + win + 1)[0])


def test_local_attn_zero_rate_is_the_plain_call():
    (q, k, v, rp, go, scale), _, _ = _local_case(2, 34, 2, 4, 5, True, 0.5)

    def run(**kw):
        leaves = [x.cuda().requires_grad_() for x in (q, k, v, rp)]
        out = T.local_attn(leaves[0], leaves[1], leaves[2], 2, 5, scale, leaves[3], **kw)
        out.backward(go.cuda())
        return [out.detach()] + [x.grad for x in leaves]
    for a, b in zip(run(), run(dropout_p=0.0, seed=SEED)):
        assert torch.equal(a, b)


# ---- channel attention -------------------------------------------------------------------------------------------------------------
# (B, C, n_head, T): hs = 17 (one 16-block and a remainder, one head) and hs = 68 (two heads, several score slices)
CHAN_SHAPES = [(2, 17, 1, 35), (2, 136, 2, 432)]


@functools.lru_cache(maxsize=None)
def _chan_case(b, c, nh, t, p):
    q, k, v, go = (seeded((b, c, t), 3 * t + c + i) for i in range(4))
    scale = 1.0 / math.sqrt(c // nh)
    m = A.factors(SEED + c, b * nh, c // nh, c // nh, p)
    fn = lambda q_, k_, v_: A.chan_attn(q_, k_, v_, nh, scale, m)          # noqa: E731
    return (q, k, v, go, scale), A.autograd(fn, [q.double(), k.double(), v.double()], go.double()), A.autograd(fn, [q, k, v], go)


@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("shape", CHAN_SHAPES)
def test_chan_attn_dropout_vs_fp64(shape, p):
    b, c, nh, t = shape
    (q, k, v, go, scale), (ref, gref), (yard, gyard) = _chan_case(*shape, p)

    def run(seed, rate=p):
        leaves = [x.cuda().requires_grad_() for x in (q, k, v)]
        out = T.chan_attn(*leaves, nh, scale, dropout_p=rate, seed=seed)
        out.backward(go.cuda())
        return out.detach(), [x.grad for x in leaves]
    out, grads = run(SEED + c)
    _check(f"chan out {shape} p={p}", out, ref, yard, C.ATTN_TOL, C.attn_bound)
    for name, g, r, y in zip(("dq", "dk", "dv"), grads, gref, gyard):
        _check(f"chan {name} {shape} p={p}", g, r, y, C.ATTN_TOL, C.attn_bound)
    out2, grads2 = run(SEED + c)
    assert torch.equal(out, out2) and all(torch.equal(g, g2) for g, g2 in zip(grads, grads2))
    assert not torch.equal(out, run(SEED + c + 1)[0])
    plain, zero = run(None, 0.0), run(SEED, 0.0)
    assert torch.equal(plain[0], zero[0]) and all(torch.equal(g, g2) for g, g2 in zip(plain[1], zero[1]))
    assert not torch.equal(plain[0], out)


# ---- the tiny OTPose through one training step -------------------------------------------------------------------------------------
def _model(**keys):
    """The tiny OTPose with token encoders and the given extra keys, filled like tests/test_gpu_token_attn.py's: the synthetic
    recipe for everything but the token encoders, the seeded fill of tests/token_attn_ref.py for those."""
    from otpose_amd import OTPose, tiny_cfg
    from otpose_amd import synthetic as S
    from tests import token_attn_ref as R
    cfg = tiny_cfg(8, (64, 96))
    cfg.MODEL.TOKEN_LAYERS, cfg.MODEL.FLOW_TOKEN_LAYERS = 1, 1
    for k, v in keys.items():
        cfg.MODEL[k] = v
    m = OTPose(cfg)
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


def _step(m, cfg, torch_seed, train_dropout=True):
    from otpose_amd import synthetic as S
    from otpose_amd import train as TR
    m = m.cuda().train()
    m.train_dropout = train_dropout
    x, margin = S.synthetic_clip(2, cfg.MODEL.IMAGE_SIZE)
    torch.manual_seed(torch_seed)
    outs = TR.forward_train(m, x.cuda(), margin.cuda())
    b, j, h, w = outs[0].shape
    tgt, wt = S.synthetic_targets(b, (w, h), j, sigma=1.5, seed=77)
    loss = TR.criterion(outs, tgt.cuda(), wt.cuda())
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


DROP_KEYS = dict(ATTN_PDROP=0.5, FLOW_ATTN_PDROP=0.5, TOKEN_ATTN_DROPOUT=0.5)


def test_tiny_otpose_trains_with_attention_dropout():
    loss, grads = _step(*_model(**DROP_KEYS), 5)
    assert bool(torch.isfinite(loss)) and len(grads) > 100
    for n, g in grads.items():
        assert bool(torch.isfinite(g).all()), n
    loss2, grads2 = _step(*_model(**DROP_KEYS), 5)
    assert torch.equal(loss, loss2) and sorted(grads) == sorted(grads2)
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n
    loss3, _ = _step(*_model(**DROP_KEYS), 6)
    assert not torch.equal(loss, loss3)
    # the attention dropout itself changes the step: the same torch seed without the keys
    loss4, _ = _step(*_model(), 5)
    assert not torch.equal(loss, loss4)


def test_train_dropout_false_switches_attention_dropout_off():
    loss, grads = _step(*_model(**DROP_KEYS), 5, train_dropout=False)
    base_loss, base_grads = _step(*_model(), 5, train_dropout=False)
    assert torch.equal(loss, base_loss) and sorted(grads) == sorted(base_grads)
    for n in grads:
        assert torch.equal(grads[n], base_grads[n]), n


def test_the_bf16_training_graph_applies_attention_dropout():
    m, cfg = _model(**DROP_KEYS)
    m.train_dtype = "bf16"
    loss, grads = _step(m, cfg, 5)
    m2, _ = _model()
    m2.train_dtype = "bf16"
    base, _ = _step(m2, cfg, 5)
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert not torch.equal(loss, base)
