"""Weight EMA on the GPU: ``otp_ema_update`` / ``otp_ema_update_table`` against the reference class's recorded states
(tests/golden/ema.npz, bit for bit: the arithmetic is specified - tests/ema_ref.py, tests/test_ema_host.py), and ``ModelEma`` on
the tiny OTPose: the stale-engine trap, the construction order against the flat optimizers, the hook in ``train_step_dp``."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import ema_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return R.load(np.load(os.path.join(GOLDEN, "ema.npz")))


def _scalars(decay):
    return float(decay), float(1. - decay)


def _bits_equal(t, ref):
    ref = torch.from_numpy(np.ascontiguousarray(ref))
    t = t.detach().cpu().reshape(ref.shape)
    view = torch.int32 if ref.dtype == torch.float32 else torch.int64
    return t.dtype == ref.dtype and torch.equal(t.view(view), ref.view(view))


def _table(pairs):
    """Device job table over (ema tensor, source tensor) pairs, built as ModelEma builds it."""
    from otpose_amd import hip
    L = hip.lib()
    nb, raw, prev = L.otp_ema_job_bytes(), bytearray(), None
    for e, s in pairs:
        code = hip.CONSTANTS["OTP_DTYPE_F32" if e.dtype == torch.float32 else "OTP_DTYPE_I64"]
        job = ctypes.create_string_buffer(nb)
        hip.check(L.otp_ema_job(hip.ptr(e), hip.ptr(s), e.numel(), code, prev, job), "otp_ema_job")
        raw.extend(job.raw)
        prev = job
    return torch.frombuffer(raw, dtype=torch.uint8).cuda()


@pytest.mark.parametrize("decay", R.DECAYS)
def test_table_reproduces_the_reference_on_every_tensor(fixture, decay):
    from otpose_amd import hip
    keys, start, srcs, emas = fixture
    ema = {k: torch.from_numpy(start[k].copy()).cuda() for k in keys}
    src = {k: torch.empty_like(ema[k]) for k in keys}
    table = _table([(ema[k], src[k]) for k in keys])
    d, omd = _scalars(decay)
    for i in range(R.STATES):
        for k in keys:
            src[k].copy_(torch.from_numpy(srcs[i][k]))
        hip.check(hip.lib().otp_ema_update_table(hip.ptr(table), len(keys), d, omd, hip.stream_of(table)), "otp_ema_update_table")
        bad = [k for k in keys if not _bits_equal(ema[k], emas[decay][i][k])]
        assert not bad, (decay, i + 1, bad)
        assert all(_bits_equal(src[k], srcs[i][k]) for k in keys)               # the source is only read


def _flat_run(fixture, decay, order, offset):
    """The fixture's float32 tensors concatenated in ``order`` with the pair of pointers ``offset`` floats past 16-byte alignment,
    through otp_ema_update five times; yields the flat result after each call."""
    from otpose_amd import hip
    keys, start, srcs, emas = fixture
    n = sum(start[k].size for k in order)
    guard = 8                                                                    # floats on either side that must stay as they are
    ebuf = torch.full((offset + n + 2 * guard,), 12345.0, device="cuda")
    sbuf = torch.full_like(ebuf, -54321.0)
    assert ebuf.data_ptr() % 16 == 0 and sbuf.data_ptr() % 16 == 0
    e, s = ebuf[guard + offset:][:n], sbuf[guard + offset:][:n]
    assert e.data_ptr() % 16 == 4 * offset and s.data_ptr() % 16 == 4 * offset
    e.copy_(torch.from_numpy(np.concatenate([start[k].reshape(-1) for k in order])))
    d, omd = _scalars(decay)
    for i in range(R.STATES):
        s.copy_(torch.from_numpy(np.concatenate([srcs[i][k].reshape(-1) for k in order])))
        hip.check(hip.lib().otp_ema_update(hip.ptr(e), hip.ptr(s), n, d, omd, hip.stream_of(e)), "otp_ema_update")
        assert bool((ebuf[:guard + offset] == 12345.0).all()) and bool((ebuf[guard + offset + n:] == 12345.0).all())
        yield i, e


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("backwards", [False, True])
@pytest.mark.parametrize("decay", R.DECAYS)
def test_flat_reproduces_the_reference_in_both_orders_at_every_alignment(fixture, decay, backwards, offset):
    keys, start, srcs, emas = fixture
    order = [k for k in keys if start[k].dtype == np.float32]
    if backwards:
        order = order[::-1]
    for i, e in _flat_run(fixture, decay, order, offset):
        want = np.concatenate([emas[decay][i][k].reshape(-1) for k in order])
        assert _bits_equal(e, want), (decay, backwards, offset, i + 1)


def test_flat_with_the_two_pointers_at_different_alignments(fixture):
    """Any 4-byte-aligned PAIR: the source one float further from its 16-byte boundary than the destination."""
    from otpose_amd import hip
    keys, start, srcs, emas = fixture
    k = "p4099"
    e = torch.zeros(4099 + 8, device="cuda")[2:][:4099]
    s = torch.zeros(4099 + 8, device="cuda")[3:][:4099]
    e.copy_(torch.from_numpy(start[k]))
    s.copy_(torch.from_numpy(srcs[0][k]))
    d, omd = _scalars(0.999)
    hip.check(hip.lib().otp_ema_update(hip.ptr(e), hip.ptr(s), 4099, d, omd, hip.stream_of(e)), "otp_ema_update")
    assert _bits_equal(e, emas[0.999][0][k])


def test_flat_and_table_routes_give_identical_bits():
    """The same data through both entry points, at a size that takes several passes of the flat kernel's capped grid and several
    workgroups' shares of the table: 4 * 256 * 4096 + 1029 floats, the pair 3 floats past alignment."""
    from otpose_amd import hip
    n = 4 * 256 * 4096 + 1029
    gen = torch.Generator().manual_seed(5)
    e0 = (torch.randn(n + 3, generator=gen) * torch.exp(8 * torch.randn(n + 3, generator=gen))).cuda()[3:]
    s = (torch.randn(n + 3, generator=gen) * torch.exp(8 * torch.randn(n + 3, generator=gen))).cuda()[3:]
    a, b = e0.clone(), torch.empty(n + 3, device="cuda")[3:].copy_(e0)
    assert b.data_ptr() % 16 == 12
    d, omd = _scalars(0.999)
    L = hip.lib()
    hip.check(L.otp_ema_update(hip.ptr(b), hip.ptr(s), n, d, omd, hip.stream_of(b)), "otp_ema_update")
    # the table: the same span cut into three jobs of uneven size (the middle one a single float)
    cuts = [(0, 1000003), (1000003, 1000004), (1000004, n)]
    table = _table([(a[lo:hi], s[lo:hi]) for lo, hi in cuts])
    hip.check(L.otp_ema_update_table(hip.ptr(table), len(cuts), d, omd, hip.stream_of(table)), "otp_ema_update_table")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    want = torch.tensor(d, device="cuda") * e0 + torch.tensor(omd, device="cuda") * s          # three rounded torch operations
    assert torch.equal(a.view(torch.int32), want.view(torch.int32))


# ---- ModelEma on the tiny OTPose ------------------------------------------------------------------------------------------------
def _tiny_model(**train):
    from otpose_amd import OTPose, tiny_cfg
    from otpose_amd import synthetic as S
    cfg = tiny_cfg(8, (64, 96))
    cfg.TRAIN.merge(train)
    model = OTPose(cfg)
    S.fill_synthetic_(model)
    model = model.cuda()
    x, margin = S.synthetic_clip(2, cfg.MODEL.IMAGE_SIZE)
    return cfg, model, x.cuda(), margin.cuda()


def _formula(old, new, decay):
    """decay * old + (1 - decay) * new as the reference writes it: three torch operations on the tensors' own device, the result
    copied into the entry's dtype."""
    out = {}
    for k in old:
        out[k] = torch.empty_like(old[k]).copy_(decay * old[k] + (1. - decay) * new[k])
    return out


def _snapshot(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _perturb_(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if v.dtype == torch.int64:
                v.add_(3)
            else:
                v.mul_((1 + 0.05 * torch.randn(v.shape, generator=gen)).to(v.device))
                v.add_((0.001 * torch.randn(v.shape, generator=gen)).to(v.device))
            if "running_var" in k:
                v.abs_()


def test_model_ema_serves_the_averaged_weights_not_a_stale_engine():
    from otpose_amd import ModelEma
    _, model, x, margin = _tiny_model()
    model.eval()
    ema = ModelEma(model, decay=0.5)
    assert type(ema.module) is type(model) and not ema.module.training
    with pytest.raises(NotImplementedError):
        ModelEma(model, device="cpu")
    with torch.no_grad():
        old_out = [o.clone() for o in model(x, margin=margin)]
        ema.set(model)
        ema_out = [o.clone() for o in ema.module(x, margin=margin)]             # (the copy now holds an engine)
    assert len(old_out) == 7
    for i, (a, b) in enumerate(zip(ema_out, old_out)):
        assert torch.equal(a, b), i
    old = _snapshot(model)
    assert all(torch.equal(v, old[k]) for k, v in ema.module.state_dict().items())
    _perturb_(model, 11)
    new = _snapshot(model)
    ema.update(model)
    want = _formula(old, new, 0.5)
    got = ema.module.state_dict()
    bad = [k for k in want if got[k].dtype != want[k].dtype or not torch.equal(got[k], want[k])]
    assert not bad, bad[:5]
    assert any(not torch.equal(want[k], old[k]) for k in want if want[k].dtype == torch.int64)      # the counters moved too
    with torch.no_grad():
        new_out = [o.clone() for o in model(x, margin=margin)]
        avg_out = [o.clone() for o in ema.module(x, margin=margin)]
    assert not torch.equal(new_out[0], old_out[0])
    # a copy that kept its packed weights would repeat old_out here
    assert not torch.equal(avg_out[0], old_out[0]) and not torch.equal(avg_out[0], new_out[0])
    assert bool(torch.isfinite(avg_out[0]).all())


def _grads_(model, seed):
    gen = torch.Generator().manual_seed(seed)
    for p in model.parameters():
        if p.requires_grad:
            p.grad = (1e-2 * torch.randn(p.shape, generator=gen)).to(p.device)


def _ema_after_one_step(ema_first):
    from otpose_amd import FusedAdamW, ModelEma
    _, model, _, _ = _tiny_model()
    if ema_first:
        ema = ModelEma(model, decay=0.9)
        ema.update(model)                                                        # a table over the parameters' first homes
        opt = FusedAdamW(model.parameters(), lr=1e-2)                            # ... which re-points param.data
    else:
        opt = FusedAdamW(model.parameters(), lr=1e-2)
        ema = ModelEma(model, decay=0.9)
        ema.update(model)
    start = _snapshot(model)
    _grads_(model, 3)
    opt.step()
    with torch.no_grad():
        for b in model.buffers():
            if b.dtype == torch.float32:
                b.add_(0.125)                                                    # the running statistics moved as well
    ema.update(model)
    assert any(not torch.equal(v, start[k]) for k, v in model.state_dict().items() if v.dtype == torch.float32)
    return ema, model, start


def test_optimizer_built_after_the_ema_leaves_no_stale_pointer():
    ema_a, model_a, start_a = _ema_after_one_step(ema_first=True)
    ema_b, model_b, start_b = _ema_after_one_step(ema_first=False)
    sd_a, sd_b = ema_a.module.state_dict(), ema_b.module.state_dict()
    assert all(torch.equal(model_a.state_dict()[k], v) for k, v in model_b.state_dict().items())
    bad = [k for k in sd_b if not torch.equal(sd_a[k], sd_b[k])]
    assert not bad, bad[:5]
    # and both are the formula on the weights after the step (the first update() averaged a state with itself)
    want = _formula(_formula(start_b, start_b, 0.9), _snapshot(model_b), 0.9)
    bad = [k for k in want if not torch.equal(sd_b[k], want[k])]
    assert not bad, bad[:5]
    # the parameters of the flat optimizer went through ONE flat launch into a mirror of the same layout
    plan = ema_a._plan
    assert plan["single"] is not None and plan["single"][2] == sum(p.numel() for p in model_a.parameters() if p.requires_grad)
    # load_state_dict copies in place: the plan stays, the update stays right
    table = plan["table"]
    model_a.load_state_dict({k: v + 1 if v.dtype == torch.float32 else v for k, v in model_a.state_dict().items()})
    before = _snapshot(ema_a.module)
    ema_a.update(model_a)
    assert ema_a._plan["table"] is table
    want = _formula(before, _snapshot(model_a), 0.9)
    assert all(torch.equal(v, want[k]) for k, v in ema_a.module.state_dict().items())


def test_train_step_dp_updates_the_ema_after_the_optimizer():
    from otpose_amd import ModelEma, make_optimizer, parallel
    from tests.test_gpu_train_e2e import _targets
    losses, states = {}, {}
    for with_ema in (False, True):
        cfg, model, x, margin = _tiny_model(OPTIMIZER="AdamW", LR=1e-3, WD=0.01)
        model.train()
        model.train_dropout = False
        model.train_dtype = "f32"
        J, (w, h) = cfg.MODEL.NUM_JOINTS, cfg.MODEL.HEATMAP_SIZE
        g, wt = _targets(2, J, h, w)
        g, wt = g.cuda(), wt.cuda()
        ema = ModelEma(model, decay=0.9) if with_ema else None                   # before the optimizer flattens the parameters
        opt = make_optimizer(model, cfg)
        cur = _snapshot(model)
        losses[with_ema] = []
        for _ in range(2):
            if with_ema:
                losses[with_ema].append(parallel.train_step_dp(model, opt, x, margin, g, wt, ema=ema))
                cur = _formula(cur, _snapshot(model), 0.9)
            else:
                losses[with_ema].append(parallel.train_step_dp(model, opt, x, margin, g, wt))
        states[with_ema] = _snapshot(model)
        if with_ema:
            got = ema.module.state_dict()
            bad = [k for k in cur if not torch.equal(got[k], cur[k])]
            assert not bad, bad[:5]
            assert not ema.module.training and ema.module._engine is None
    for a, b in zip(losses[False], losses[True]):
        assert torch.equal(a, b), (float(a), float(b))
    assert all(torch.equal(v, states[True][k]) for k, v in states[False].items())
