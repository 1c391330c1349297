"""Fused clip + SGD (otp_grad_sumsq / otp_sgd_step, ``FusedSGD``) vs torch.nn.utils.clip_grad_norm_ + torch.optim.SGD on the
CPU, and the training set-up built from cfg (``make_optimizer`` / ``make_scheduler``) inside ``parallel.train_step_dp``.

Bound of the arithmetic tests: 2e-6 * max(1, max|ref|), the one tests/test_gpu_optim.py holds AdamW to - at most six fp32
roundings per element and step (clip * g, + wd * p, momentum * buf, + (1 - dampening) * d, + momentum * buf, p - lr * d) over
4 steps: 24 * 2^-24 = 1.4e-6."""
import copy
import json
import os

import pytest
import torch

from tests.conftest import GOLDEN, seeded

pytestmark = pytest.mark.gpu

BOUND = 2e-6
BIG_N = 4 * 256 * 4096 + 4 * 256 + 3      # one full pass of the capped grid, a second partial pass, a 3-element tail


def _close(a, b, what):
    a = a.detach().cpu()
    err = float((a - b.detach()).abs().max())
    assert err <= BOUND * max(1.0, float(b.detach().abs().max())), (what, err)


def _params():
    """Three groups: flat lengths 3 (the scalar tail alone), 41 (vector part + tail) and 48 (vector part alone)."""
    shapes = [[(3,)], [(5, 7), (6,)], [(8, 4), (16,)]]
    return [[torch.nn.Parameter(seeded(s, 40 + 7 * gi + i)) for i, s in enumerate(g)] for gi, g in enumerate(shapes)]


def _groups(params, lr):
    return [{"params": params[0], "lr": lr / 100, "weight_decay": 0.05}, {"params": params[1], "weight_decay": 0.0},
            {"params": params[2], "weight_decay": 0.01}]


def _feed(ref, dut, seed, scale=0.1):
    """Identical gradients on both sides (the optimizer arithmetic is under test, not a backward)."""
    gen = torch.Generator().manual_seed(seed)
    for a, b in zip(ref, dut):
        g = torch.randn(a.shape, generator=gen) * scale
        a.grad = g.clone()
        b.grad = g.cuda()                                    # an ordinary tensor: step() copies it into the flat slot


@pytest.mark.parametrize("max_norm", [0.0, 0.05])
@pytest.mark.parametrize("momentum,dampening,nesterov", [(0, 0, False), (0.9, 0, False), (0.9, 0, True), (0.9, 0.1, False)])
def test_fused_sgd_matches_torch(momentum, dampening, nesterov, max_norm):
    from otpose_amd.optim import FusedSGD
    ref = _params()
    dut = [[torch.nn.Parameter(p.detach().clone().cuda()) for p in g] for g in ref]
    lr = 3e-2
    kw = dict(lr=lr, momentum=momentum, dampening=dampening, nesterov=nesterov)
    o_ref = torch.optim.SGD(_groups(ref, lr), **kw)
    o_dut = FusedSGD(_groups(dut, lr), max_grad_norm=max_norm, **kw)
    assert [f["p"].numel() for f in o_dut._flat] == [3, 41, 48]
    flat_ref, flat_dut = [p for g in ref for p in g], [p for g in dut for p in g]
    versions = [p._version for p in flat_dut]
    for it in range(4):
        o_ref.zero_grad()
        o_dut.zero_grad()
        _feed(flat_ref, flat_dut, 10 + it)
        if max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_(flat_ref, max_norm)
            assert abs(float(o_dut.grad_norm()) - float(total)) <= 1e-5 * float(total)
            assert float(total) > max_norm                  # the clip is active
        o_ref.step()
        o_dut.step()
        for i, (a, b) in enumerate(zip(flat_ref, flat_dut)):
            _close(b, a, ("param", it, i))
            if momentum:
                buf = o_dut.state[b]["momentum_buffer"]
                _close(buf, o_ref.state[a]["momentum_buffer"], ("momentum_buffer", it, i))
            else:
                assert "momentum_buffer" not in o_dut.state[b]
    assert all(p._version > v for p, v in zip(flat_dut, versions))      # staleness checks see the update
    for f in o_dut._flat:
        if momentum:
            lo, hi = f["b"].data_ptr(), f["b"].data_ptr() + 4 * f["b"].numel()
            assert all(lo <= o_dut.state[p]["momentum_buffer"].data_ptr() < hi for p in f["params"])
        else:
            assert f["b"] is None                             # momentum == 0 allocates and touches no buffer


def test_fused_sgd_rejects_what_torch_rejects():
    from otpose_amd.optim import FusedSGD
    p = [torch.nn.Parameter(torch.zeros(4, device="cuda"))]
    for kw in (dict(lr=-1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-0.1),
               dict(lr=0.1, nesterov=True), dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError):
            torch.optim.SGD(p, **kw)
        with pytest.raises(ValueError):
            FusedSGD(p, **kw)
    with pytest.raises(RuntimeError):
        FusedSGD([torch.nn.Parameter(torch.zeros(4))], lr=0.1)                                  # not on the GPU
    with pytest.raises(RuntimeError):
        FusedSGD([torch.nn.Parameter(torch.zeros(4, device="cuda", dtype=torch.float64))], lr=0.1)


@pytest.fixture(scope="module")
def big():
    """One parameter that needs the grid-stride loop and the tail, two gradients, and two CPU steps of torch.optim.SGD."""
    p0 = seeded((BIG_N,), 5)
    grads = [seeded((BIG_N,), 6, 1e-3), seeded((BIG_N,), 7, 1e-3)]
    kw = dict(lr=0.05, momentum=0.9, weight_decay=0.01)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([ref], **kw)
    after = []
    for g in grads:
        ref.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([ref], 1.0)
        assert float(total) > 1.0                           # the clip is active
        opt.step()
        after.append((ref.detach().clone(), opt.state[ref]["momentum_buffer"].clone()))
    return p0, grads, kw, after


def _run_big(big):
    from otpose_amd.optim import FusedSGD
    p0, grads, kw, _ = big
    p = torch.nn.Parameter(p0.cuda())
    opt = FusedSGD([p], max_grad_norm=1.0, **kw)
    out = []
    for g in grads:
        opt.zero_grad()
        p.grad = g.cuda()
        opt.step()
        out.append((p.detach().clone(), opt.state[p]["momentum_buffer"].clone()))
    return out


def test_grid_stride_loop_and_tail(big):
    for it, ((p, b), (rp, rb)) in enumerate(zip(_run_big(big), big[3])):
        _close(p, rp, ("param", it))
        _close(b, rb, ("momentum_buffer", it))
        # the ends of every region of the launch: first / last vector of the first pass, the second pass, the tail
        for i in (0, 4 * 256 * 4096 - 1, 4 * 256 * 4096, BIG_N - 4, BIG_N - 3, BIG_N - 1):
            assert abs(float(p[i]) - float(rp[i])) <= BOUND * max(1.0, abs(float(rp[i]))), (it, i)


def test_same_bits_on_every_run(big):
    first, second = _run_big(big), _run_big(big)
    for (p1, b1), (p2, b2) in zip(first, second):
        assert torch.equal(p1, p2) and torch.equal(b1, b2)


def _grads(params, seed, scale=0.1):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(p.shape, generator=gen) * scale for p in params]


def test_state_interchange_with_torch_sgd():
    from otpose_amd.optim import FusedSGD
    lr, kw = 3e-2, dict(momentum=0.9, dampening=0.1)
    ref = _params()
    flat_ref = [p for g in ref for p in g]
    o_ref = torch.optim.SGD(_groups(ref, lr), lr=lr, **kw)
    for it in range(2):
        for p, g in zip(flat_ref, _grads(flat_ref, 20 + it)):
            p.grad = g
        o_ref.step()
    dut = [[torch.nn.Parameter(p.detach().clone().cuda()) for p in g] for g in ref]
    flat_dut = [p for g in dut for p in g]
    o_dut = FusedSGD(_groups(dut, lr), lr=lr, **kw)
    assert all(f["first"] for f in o_dut._flat)
    o_dut.load_state_dict(copy.deepcopy(o_ref.state_dict()))
    assert not any(f["first"] for f in o_dut._flat)          # a state with buffers is past its first step
    for f in o_dut._flat:
        lo, hi = f["b"].data_ptr(), f["b"].data_ptr() + 4 * f["b"].numel()
        assert all(lo <= o_dut.state[p]["momentum_buffer"].data_ptr() < hi for p in f["params"])
    for it in range(2):
        for a, b, g in zip(flat_ref, flat_dut, _grads(flat_ref, 30 + it)):
            a.grad, b.grad = g.clone(), g.cuda()
        o_ref.step()
        o_dut.step()
        for i, (a, b) in enumerate(zip(flat_ref, flat_dut)):
            _close(b, a, ("param", it, i))
            _close(o_dut.state[b]["momentum_buffer"], o_ref.state[a]["momentum_buffer"], ("momentum_buffer", it, i))
    # and back: a fresh torch.optim.SGD over CPU copies takes FusedSGD's state
    back = [[torch.nn.Parameter(p.detach().cpu().clone()) for p in g] for g in dut]
    o_back = torch.optim.SGD(_groups(back, lr), lr=lr, **kw)
    sd = o_dut.state_dict()
    assert [g["lr"] for g in sd["param_groups"]] == [lr / 100, lr, lr]
    o_back.load_state_dict(sd)
    for a, b in zip([p for g in back for p in g], flat_dut):
        assert torch.equal(o_back.state[a]["momentum_buffer"], o_dut.state[b]["momentum_buffer"].cpu())
    # before its first step FusedSGD has, like torch, no buffers to hand over
    fresh = FusedSGD(_groups([[torch.nn.Parameter(p.detach().clone()) for p in g] for g in dut], lr), lr=lr, **kw)   # (GPU copies)
    assert fresh.state_dict()["state"] == {}


# ---- inside the training step ---------------------------------------------------------------------------------------------
def _tiny(optimizer, **train):
    from otpose_amd import OTPose, tiny_cfg
    from otpose_amd import synthetic as S
    cfg = tiny_cfg(8, (64, 96))
    cfg.TRAIN.merge(dict(train, OPTIMIZER=optimizer))
    model = OTPose(cfg)
    S.fill_synthetic_(model)
    model = model.cuda().train()
    model.train_dropout = False
    model.train_dtype = "f32"
    x, margin = S.synthetic_clip(2, cfg.MODEL.IMAGE_SIZE)
    return cfg, model, x.cuda(), margin.cuda()


def test_sgd_and_schedule_in_the_training_step():
    """``make_optimizer`` (SGD: fused by default on the GPU) + ``make_scheduler`` (warm-up + cosine, 3 iterations per epoch)
    through ``parallel.train_step_dp``, on the model and inputs of test_gpu_train_e2e.py::test_train_step_matches_oracle_autograd."""
    from otpose_amd import make_optimizer, make_scheduler, parallel
    from otpose_amd.optim import FusedSGD
    from tests.test_gpu_train_e2e import _targets
    with open(os.path.join(GOLDEN, "lr_schedule.json")) as f:
        table = json.load(f)
    cfg, model, x, margin = _tiny("SGD", LR=table["base_lrs"][0], WARMUP=True, LR_SCHEDULER="CosineAnnealingLR", **table["train"])
    J, (w, h) = cfg.MODEL.NUM_JOINTS, cfg.MODEL.HEATMAP_SIZE
    g, wt = _targets(2, J, h, w)
    g, wt = g.cuda(), wt.cuda()
    opt = make_optimizer(model, cfg)
    assert type(opt) is FusedSGD and opt.max_grad_norm == 1.0
    assert [grp["momentum"] for grp in opt.param_groups] == [cfg.TRAIN.MOMENTUM] * 3
    assert [grp["lr"] for grp in opt.param_groups] == table["base_lrs"]
    sched = make_scheduler(opt, cfg, table["iters_per_epoch"])
    ref_lr = table["lr"]["warmup_CosineAnnealingLR"]
    trainable = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    group_of = {id(p): gi for gi, grp in enumerate(opt.param_groups) for p in grp["params"]}
    for it in range(3):
        lrs = [grp["lr"] for grp in opt.param_groups]
        for gi, lr in enumerate(lrs):
            assert abs(lr - ref_lr[gi][it]) <= 1e-12 * ref_lr[gi][it], (it, gi, lr)
        before = [p.detach().clone() for _, p in trainable]
        loss = parallel.train_step_dp(model, opt, x, margin, g, wt, scheduler=sched)
        assert bool(torch.isfinite(loss).all()), (it, float(loss))
        # the backward kernels wrote into the flat buffer: every gradient is its slot
        assert all(p.grad is not None and p.grad.data_ptr() == p._otp_grad_slot.data_ptr() for _, p in trainable), it
        same = [n for (n, p), p0 in zip(trainable, before) if torch.equal(p.detach(), p0)]
        print("step %d: lr %s, loss %.6f, %d of %d trainable tensors unchanged" % (it + 1, lrs, float(loss), len(same), len(trainable)))
        if it == 0:
            assert len(same) == len(trainable)              # step 1 runs at rate 0
        if it == 1:
            # Step 2 moves every trainable parameter - as far as float32 can show it.  The clip scales this fixture's gradient
            # (norm ~2e3) to norm 1 and the rate is 2e-5 (2e-7 for the backbone), so for most tensors lr * buf is below half
            # an ulp of every weight (on the CPU, with the oracle's gradients: 1251 of 1696 tensors, and 199 even at LR = 1).
            # So each tensor is held to its own update: p_after = p_before - lr * momentum_buffer within the arithmetic
            # bound, and it must differ from p_before wherever one element's step exceeds 2^-23 |p| (>= one ulp: it cannot
            # round away, fused multiply-add or not).
            moved_by_group, must = [0, 0, 0], 0
            for (n, p), p0 in zip(trainable, before):
                gi = group_of[id(p)]
                upd = lrs[gi] * opt.state[p]["momentum_buffer"]
                want = p0 - upd
                err = float((p.detach() - want).abs().max())
                assert err <= BOUND * max(1.0, float(want.abs().max())), (n, err)
                changed = not torch.equal(p.detach(), p0)
                moved_by_group[gi] += changed
                if bool((upd.abs() > 2.0 ** -23 * p0.abs()).any()):
                    must += 1
                    assert changed, n
            print("step 2: tensors that moved per group %s, %d had a step of at least one ulp" % (moved_by_group, must))
            assert all(m > 0 for m in moved_by_group) and must > 0
    for gi, grp in enumerate(opt.param_groups):
        assert abs(grp["lr"] - ref_lr[gi][3]) <= 1e-12 * ref_lr[gi][3]
    # straight after a backward (no step() in between): autograd adopted the slot views the kernels wrote into
    opt.zero_grad()
    from otpose_amd import train as TR
    TR.criterion(TR.forward_train(model, x, margin), g, wt).backward()
    adopted = sum(1 for _, p in trainable if p.grad is not None and p.grad.data_ptr() == p._otp_grad_slot.data_ptr())
    print("adopted straight after the backward: %d of %d" % (adopted, len(trainable)))
    assert adopted > 0.9 * len(trainable), adopted           # the share tests/test_gpu_train_slots.py asks of FusedAdamW


def test_adamw_through_the_factory_reproduces_the_reference_step(golden):
    """One step with ``make_optimizer(model, cfg)`` (AdamW, fused, clip 1.0) against the weights the reference moved with its
    own ``make_optimizer`` groups (tests/golden/train_step_tiny.npz, ``step/*`` = weight after - before; LR 1e-3, WD 0.01).
    tests/test_gpu_train_e2e.py does not read that golden; what it holds the fp32 step's per-tensor results to against its
    reference is TOL["f32"]: relative L2 error ``rel`` and cosine ``cos`` per tensor - read from there and applied to each
    recorded weight step."""
    from otpose_amd import make_optimizer, parallel
    from otpose_amd.optim import FusedAdamW
    from tests.test_gpu_train_e2e import TOL
    gd = golden("train_step_tiny")
    cfg, model, x, margin = _tiny("AdamW", LR=1e-3, WD=0.01)
    opt = make_optimizer(model, cfg)
    assert type(opt) is FusedAdamW and opt.max_grad_norm == 1.0
    assert [len(grp["params"]) for grp in opt.param_groups] == gd["opt_group_sizes"].tolist()
    assert [grp["lr"] for grp in opt.param_groups] == gd["opt_group_lr"].tolist()
    assert [grp["weight_decay"] for grp in opt.param_groups] == gd["opt_group_wd"].tolist()
    keys = [k[5:] for k in gd if k.startswith("step/")]
    assert len(keys) == 5
    named = dict(model.named_parameters())
    before = {k: named[k].detach().clone() for k in keys}
    parallel.train_step_dp(model, opt, x, margin, gd["target"].cuda(), gd["target_weight"].cuda())
    bad = []
    for k in keys:
        ref = gd["step/" + k].double()
        mine = (named[k].detach() - before[k]).cpu().double()
        rel = float((mine - ref).norm() / ref.norm())
        cos = float((mine * ref).sum() / (mine.norm() * ref.norm()))
        print("weight step %s: rel L2 err %.3e, cosine %.6f, |ref| %.3e" % (k, rel, cos, float(ref.norm())))
        if rel > TOL["f32"]["rel"] or cos < TOL["f32"]["cos"]:
            bad.append((k, rel, cos))
    assert not bad, bad
