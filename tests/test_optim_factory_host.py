"""Training set-up from cfg, host side: ``make_optimizer``'s three groups against the reference's (recorded in
tests/golden/state_dict_w32.json), ``make_scheduler``'s four branches against the learning rates the reference's own
schedulers produced (tests/golden/lr_schedule.json, written by tests/golden/make_optim_golden.py), and the argument checks
of otp_sgd_step, which return before anything touches a GPU."""
import ctypes
import json
import os

import pytest
import torch

from otpose_amd import CfgNode, OTPose, cfg1, hip, make_optimizer, make_scheduler
from otpose_amd import schedule as SCH
from tests.conftest import GOLDEN


def _json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


# ---- make_optimizer -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def w32():
    return OTPose(cfg1())


@pytest.mark.parametrize("name,cls", [("AdamW", torch.optim.AdamW), ("SGD", torch.optim.SGD)])
def test_groups_match_reference(w32, name, cls):
    ref = _json("state_dict_w32.json")["w32"]["optimizer_groups"]
    cfg = cfg1()
    cfg.TRAIN.merge({"OPTIMIZER": name, "LR": 2e-4, "WD": 0.01, "MOMENTUM": 0.8, "NESTEROV": True})
    opt = make_optimizer(w32, cfg, fused=False)
    assert type(opt) is cls
    names = {id(p): n for n, p in w32.named_parameters()}
    groups = opt.param_groups
    assert len(groups) == 3
    for g, key, count in zip(groups, ("decay", "no_decay", "pretrained"), (315, 503, 878)):
        mine = [names[id(p)] for p in g["params"]]
        assert mine == sorted(mine)                               # each group is ordered by full parameter name
        assert mine == ref[key] and len(mine) == count
    assert [g["lr"] for g in groups] == [2e-4, 2e-4, 2e-4 / 100]
    assert [g["weight_decay"] for g in groups] == [0.01, 0.0, 0.01]
    if name == "SGD":
        assert all(g["momentum"] == 0.8 and g["nesterov"] is False and g["dampening"] == 0 for g in groups)   # NESTEROV is not read
    else:
        assert all(g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 for g in groups)


def test_frozen_backbone_stays_in_its_group():
    m = OTPose(cfg1())
    m.rough_pose_estimation_net.freeze_weight()
    opt = make_optimizer(m, cfg1(), fused=False)
    assert [len(g["params"]) for g in opt.param_groups] == [315, 503, 878]
    assert not any(p.requires_grad for p in opt.param_groups[2]["params"])


def test_unknown_optimizer(w32):
    cfg = cfg1()
    cfg.TRAIN.OPTIMIZER = "Adam"
    with pytest.raises(TypeError, match="Unsupported optimizer!"):
        make_optimizer(w32, cfg, fused=False)


def test_fused_needs_a_gpu(w32):
    with pytest.raises(RuntimeError):
        make_optimizer(w32, cfg1(), fused=True)                   # CPU parameters: no quiet fall-back to torch.optim


# ---- make_scheduler -----------------------------------------------------------------------------------------------------
def _sched_cfg(table, warmup, name):
    return CfgNode({"TRAIN": dict(table["train"], WARMUP=warmup, LR_SCHEDULER=name)})


def _dummy_optimizer(kind, base_lrs):
    groups = [{"params": [torch.nn.Parameter(torch.zeros(2))], "lr": lr} for lr in base_lrs]
    return torch.optim.SGD(groups, lr=base_lrs[0]) if kind == "SGD" else torch.optim.AdamW(groups, lr=base_lrs[0])


def _assert_lr(mine, ref, rel, where):
    if ref == 0.0:
        assert abs(mine) <= 1e-20, (where, mine, ref)
    else:
        assert abs(mine - ref) <= rel * abs(ref), (where, mine, ref)


@pytest.mark.parametrize("kind", ["SGD", "AdamW"])
@pytest.mark.parametrize("name", ["CosineAnnealingLR", "MultiStepLR"])
@pytest.mark.parametrize("warmup", [True, False])
def test_lr_table_matches_reference(warmup, name, kind):
    table = _json("lr_schedule.json")
    ref = table["lr"][("warmup_" if warmup else "plain_") + name]
    opt = _dummy_optimizer(kind, table["base_lrs"])
    sched = make_scheduler(opt, _sched_cfg(table, warmup, name), table["iters_per_epoch"])
    assert isinstance(sched, torch.optim.lr_scheduler.LRScheduler)
    if warmup:
        assert type(sched) is (SCH.LinearWarmupCosineAnnealingLR if name == "CosineAnnealingLR" else SCH.LinearWarmupMultiStepLR)
    for it in range(table["iterations"]):
        for gi, g in enumerate(opt.param_groups):
            _assert_lr(g["lr"], ref[gi][it], 1e-12, (it, gi))
        opt.step()
        sched.step()
    if name == "MultiStepLR":                                     # the reference's empty milestone list: GAMMA is never applied
        assert [g["lr"] for g in opt.param_groups] == table["base_lrs"]


@pytest.mark.parametrize("name", ["CosineAnnealingLR", "MultiStepLR"])
def test_closed_form_agrees_with_chainable(name):
    table = _json("lr_schedule.json")
    ref = table["lr"]["warmup_" + name]
    cfg = _sched_cfg(table, True, name)
    sched = make_scheduler(_dummy_optimizer("SGD", table["base_lrs"]), cfg, table["iters_per_epoch"])
    max_steps = (cfg.TRAIN.END_EPOCH + cfg.TRAIN.WARMUP_EPOCHS) * table["iters_per_epoch"]
    for it in range(max_steps + 1):                               # the warm-up and the first cosine period
        sched.last_epoch = it
        for gi, lr in enumerate(sched._get_closed_form_lr()):
            _assert_lr(lr, ref[gi][it], 1e-9, ("closed form", it, gi))
    opt = _dummy_optimizer("SGD", table["base_lrs"])
    sched = make_scheduler(opt, cfg, table["iters_per_epoch"])
    with pytest.warns(UserWarning):                               # torch's deprecation warning of step(epoch)
        sched.step(7)
    for gi, g in enumerate(opt.param_groups):
        _assert_lr(g["lr"], ref[gi][7], 1e-9, ("step(7)", gi))


def test_multistep_milestones_when_given():
    """The class itself (the factory never hands it a milestone): chainable and closed form decay alike."""
    opt = _dummy_optimizer("SGD", [1e-2])
    sched = SCH.LinearWarmupMultiStepLR(opt, 3, [2, 4, 4], gamma=0.5)
    seen = []
    for _ in range(9):
        seen.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    want = [0.0, 5e-3, 1e-2, 1e-2, 1e-2, 5e-3, 5e-3, 1.25e-3, 1.25e-3]
    assert seen == pytest.approx(want, rel=1e-12, abs=0)
    for it, lr in enumerate(want):
        sched.last_epoch = it
        assert sched._get_closed_form_lr()[0] == pytest.approx(lr, rel=1e-12, abs=0)


def test_unknown_scheduler():
    table = _json("lr_schedule.json")
    for warmup in (True, False):
        with pytest.raises(TypeError, match="Unsupported scheduler!"):
            make_scheduler(_dummy_optimizer("SGD", [1e-4]), _sched_cfg(table, warmup, "StepLR"), 3)


def test_train_step_dp_steps_the_scheduler():
    """``parallel.train_step_dp(..., scheduler=s)`` steps ``s`` once, behind the optimizer; without it nothing changes."""
    from otpose_amd import parallel
    table = _json("lr_schedule.json")
    lin = torch.nn.Linear(3, 2)
    opt = torch.optim.SGD(lin.parameters(), lr=1e-4, momentum=0.9)
    sched = make_scheduler(opt, _sched_cfg(table, True, "CosineAnnealingLR"), table["iters_per_epoch"])
    x, t = torch.ones(4, 3), torch.zeros(4, 17, 2, 1)
    fwd = lambda m, x_, margin: m(x_)                                                       # noqa: E731
    crit = lambda out, tgt, w, flags: (out ** 2).mean()                                     # noqa: E731
    before = [p.detach().clone() for p in lin.parameters()]
    parallel.train_step_dp(lin, opt, x, None, t, None, forward=fwd, criterion=crit, scheduler=sched)
    assert sched.last_epoch == 1 and opt.param_groups[0]["lr"] == table["lr"]["warmup_CosineAnnealingLR"][0][1]
    assert all(torch.equal(a, b) for a, b in zip(before, lin.parameters()))                # the first step runs at rate 0
    parallel.train_step_dp(lin, opt, x, None, t, None, forward=fwd, criterion=crit)
    assert sched.last_epoch == 1
    assert not any(torch.equal(a, b) for a, b in zip(before, lin.parameters()))


# ---- otp_sgd_step: argument checks --------------------------------------------------------------------------------------
BAD_ARG, UNSUPPORTED = hip.CONSTANTS["OTP_ERR_BAD_ARG"], hip.CONSTANTS["OTP_ERR_UNSUPPORTED"]
P = ctypes.c_void_p


def _sgd(param=0x1000, grad=0x2000, buf=0x3000, n=64, lr=0.1, momentum=0.9, dampening=0.0, wd=0.0, nesterov=0, first=1):
    """Every call here is rejected before the launch, so the addresses are never read."""
    return hip.lib().otp_sgd_step(P(param), P(grad), P(buf), n, lr, momentum, dampening, wd, nesterov, first, None, 0.0, None)


def test_sgd_step_is_bound_from_the_header():
    res, args = hip.SIGNATURES["otp_sgd_step"]
    assert res is ctypes.c_int
    assert args == [P, P, P, ctypes.c_size_t] + [ctypes.c_float] * 4 + [ctypes.c_int] * 2 + [P, ctypes.c_float, P]


@pytest.mark.parametrize("kw,code", [
    (dict(param=None), BAD_ARG), (dict(grad=None), BAD_ARG), (dict(n=0), BAD_ARG),
    (dict(buf=None), BAD_ARG),                                             # momentum != 0 needs a buffer
    (dict(nesterov=1, momentum=0.0), BAD_ARG), (dict(nesterov=1, dampening=0.1), BAD_ARG),
    (dict(lr=-0.1), BAD_ARG), (dict(momentum=-0.9), BAD_ARG), (dict(wd=-0.01), BAD_ARG),
    (dict(param=0x1004), UNSUPPORTED), (dict(grad=0x2008), UNSUPPORTED), (dict(buf=0x300c), UNSUPPORTED),
    (dict(param=0x1004, momentum=0.0, buf=None), UNSUPPORTED),            # momentum == 0 takes a null buffer: alignment is next
])
def test_sgd_step_rejects(kw, code):
    assert _sgd(**kw) == code
