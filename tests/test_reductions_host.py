"""tests/reductions_ref.py pinned on the CPU: each float64 reference against torch double autograd, ``F.batch_norm``,
``torch.optim.AdamW`` on double parameters or ``clip_grad_norm_``; and the properties of the shared inputs
(tests/reductions_cases.py) that tests/test_gpu_train_reductions.py relies on - mixed flags, separated top-k losses, fp32
yardsticks inside the existing tolerances, bf16 roundings of the fp32 yardstick inside the one-step allowance."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import reductions_cases as K
from tests import reductions_ref as R

D = torch.float64


def _eq(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("relu,with_res", [(True, True), (True, False), (False, True), (False, False)])
def test_bn_reference_matches_double_autograd(relu, with_res):
    d = {k: v.double() for k, v in K.bn_inputs(3, 5, 7).items()}
    x, g, b, res = (d[k].clone().requires_grad_() for k in ("x", "gamma", "beta", "res"))
    rm, rv = d["rm"].clone(), d["rv"].clone()
    y = F.batch_norm(x, rm, rv, g, b, True, 0.1, 1e-5)
    if with_res:
        y = y + res
    if relu:
        y = F.relu(y)
    y.backward(d["dy"])
    f = R.bn_train_forward(d["x"], d["gamma"], d["beta"], d["res"] if with_res else None, d["rm"], d["rv"], 0.1, 1e-5, relu)
    _eq(f["y"], y.detach())
    _eq(f["running_mean"], rm)
    _eq(f["running_var"], rv)
    bw = R.bn_train_backward(d["dy"], d["x"], d["gamma"], f["y"] if relu else None)
    _eq(bw["dx"], x.grad)
    _eq(bw["dgamma"], g.grad)
    _eq(bw["dbeta"], b.grad)
    if with_res:
        _eq(bw["dres"], res.grad)
    _eq(R.channel_sum(d["dy"]), d["dy"].sum(dim=(0, 2, 3)))


def test_bn_reference_single_value_per_channel():
    """count == 1: the variance is zero, y = beta, and running_var takes the biased variance (no division by zero)."""
    d = K.bn_inputs(1, 3, 1)
    f = R.bn_train_forward(d["x"], d["gamma"], d["beta"], None, d["rm"], d["rv"], 0.1, 1e-5, False)
    _eq(f["y"].reshape(-1), d["beta"].double())
    _eq(f["rstd"], torch.full((3,), 1.0 / math.sqrt(1e-5), dtype=D))
    _eq(f["running_var"], 0.9 * d["rv"].double())
    _eq(f["running_mean"], 0.9 * d["rm"].double() + 0.1 * d["x"].double().reshape(-1))
    assert float(R.bn_train_backward(d["dy"], d["x"], d["gamma"]).get("dx").abs().max()) == 0.0


def test_nhwc_references_match_the_nchw_ones():
    """The finalize / backward references of the bf16 path are the NCHW ones fed with sums / a transposed layout."""
    px, c, cs = 50, 5, 8
    d = K.nhwc_bwd_inputs(px, c, cs)
    x = d["x"].double()
    part = torch.stack([x, x * x], dim=1)                                  # one pixel per row
    rm, rv = torch.zeros(c, dtype=D), torch.ones(c, dtype=D)
    beta = torch.arange(c, dtype=D)
    f = R.nhwc_bn_finalize(part, c, px, d["gamma"], beta, rm, rv)
    x4 = x.t().reshape(1, cs, px, 1)
    g8 = torch.cat([d["gamma"].double(), torch.zeros(cs - c, dtype=D)])
    ref = R.bn_train_forward(x4[:, :c], d["gamma"], beta, None, rm, rv, relu=False)
    _eq(f["mean"][:c], ref["mean"])
    _eq(f["rstd"][:c], ref["rstd"], 1e-9)
    _eq(f["running_var"], ref["running_var"], 1e-9)
    y = x4[:, :c] * f["scale"][:c].reshape(1, c, 1, 1) + f["shift"][:c].reshape(1, c, 1, 1)
    _eq(y, ref["y"], 1e-9)
    assert float(f["scale"][c:].abs().max()) == 0 and float(f["shift"][c:].abs().max()) == 0
    keep = d["y"] > 0
    mean, _, rstd, _ = R.bn_stats(x4)
    b = R.nhwc_bn_backward(d["gy"], d["x"], mean, rstd, g8, c, keep)
    y4 = d["y"].double().t().reshape(1, cs, px, 1)
    ref = R.bn_train_backward(d["gy"].double().t().reshape(1, cs, px, 1), x4, g8, y4)
    _eq(b["gx"].t().reshape(1, cs, px, 1), ref["dx"])
    _eq(b["dgamma"], ref["dgamma"][:c])
    _eq(b["dbeta"], ref["dbeta"][:c])
    assert float(b["gx"][:, c:].abs().max()) == 0


def _loss_module_st(s, t, g, w, topk, flags):
    """ST_OHKW_MSELoss written from its definition, vectorised (independent of the oracle's loop)."""
    b, j = s.shape[:2]
    s, t, g = (v.reshape(b, j, -1) for v in (s, t, g))
    a, gg, tt = s * w, g * w, t * w
    nf = (1 - flags.double()).reshape(1, j, 1)
    e = (a - gg) ** 2 + nf * (a - tt) ** 2
    l = (0.5 * e).mean(2)
    ohkm = (torch.topk(l, topk, dim=1).values.sum(1) / topk).mean()
    mse = e.mean(dim=(0, 2)).sum()
    return ohkm, mse / j, ohkm + mse


@pytest.mark.parametrize("given", [False, True])
def test_st_ohkw_reference_matches_double_autograd(given):
    b, j, hw, topk = 3, 7, 20, 3
    d = K.loss_inputs(b, j, hw)
    flags = torch.roll(d["expected_flags"], 1) if given else None
    r = R.st_ohkw(d["s"], d["t"], d["g"], d["w"], topk, flags)
    assert r["flags"].tolist() == (flags if given else d["expected_flags"]).tolist()
    s, t, g = (d[k].double().requires_grad_() for k in ("s", "t", "g"))
    ohkm, mse, final = _loss_module_st(s, t, g, d["w"].double(), topk, r["flags"])
    final.backward()
    _eq(r["ohkm_loss_s"], ohkm.detach())
    _eq(r["mse_loss_s"], mse.detach())
    _eq(r["final_loss"], final.detach())
    _eq(r["grad_s"], s.grad)
    _eq(r["grad_t"], t.grad)
    _eq(r["grad_g"], g.grad)
    _eq(r["per_sample"], R.st_ohkw_per_sample(d["s"], d["t"], d["g"], d["w"], r["flags"]))
    assert R.topk_gap(r["per_sample"], topk) > K.TOPK_GAP


@pytest.mark.parametrize("use_w,eff", [(True, None), (False, 5)])
def test_joints_references_match_double_autograd(use_w, eff):
    b, j, hw, topk = 3, 7, 20, 3
    d = K.loss_inputs(b, j, hw)
    w = d["w"] if use_w else None
    wd = d["w"].double() if use_w else torch.ones(b, j, 1, dtype=D)
    o = d["s"].double().requires_grad_()
    e = ((o.reshape(b, j, -1) - d["g"].double().reshape(b, j, -1)) * wd) ** 2
    ohkm = (torch.topk((0.5 * e).mean(2), topk, dim=1).values.sum(1) / topk).mean()
    mse = e.mean(dim=(0, 2)).sum()
    (ohkm + mse).backward()
    r = R.joints_ohkm_mse(d["s"], d["g"], w, eff, topk)
    _eq(r["ohkm_loss"], ohkm.detach())
    _eq(r["mse_loss"], mse.detach() / (eff or j))
    _eq(r["final_loss"], (ohkm + mse).detach())
    _eq(r["grad_output"], o.grad)
    o2 = d["s"].double().requires_grad_()
    v = (((o2.reshape(b, j, -1) - d["g"].double().reshape(b, j, -1)) * wd) ** 2).mean(dim=(0, 2)).sum() / (eff or j)
    v.backward()
    rv, rg = R.joint_mse(d["s"], d["g"], w, eff)
    _eq(rv, v.detach())
    _eq(rg, o2.grad)


@pytest.mark.parametrize("case", K.LOSS_CASES)
def test_loss_inputs_have_mixed_flags_and_separated_topk(case):
    b, j, hw, topk = case
    d = K.loss_inputs(b, j, hw)
    fl = R.st_ohkw_flags(d["g"])
    assert fl.tolist() == d["expected_flags"].tolist() and 0 < int(fl.sum()) < j
    assert int((d["w"] == 0).sum()) > 0 or b * j < 8
    for flags in (fl, torch.roll(fl, 1)):
        assert R.topk_gap(R.st_ohkw_per_sample(d["s"], d["t"], d["g"], d["w"], flags), topk) > K.TOPK_GAP
    assert R.topk_gap(R.joints_per_sample(d["s"], d["g"], d["w"]), topk) > K.TOPK_GAP
    assert R.topk_gap(R.joints_per_sample(d["s"], d["g"], None), topk) > K.TOPK_GAP


@pytest.mark.parametrize("max_norm", [0.0, 0.05, 1e3])
def test_adamw_reference_matches_torch_double(max_norm):
    sizes = [5, 33, 2]
    ps = [torch.nn.Parameter(K.adamw_inputs(n, i)[0].double()) for i, n in enumerate(sizes)]
    opt = torch.optim.AdamW([{"params": ps[:2], "weight_decay": 0.05}, {"params": ps[2:], "weight_decay": 0.0, "lr": 1e-4}],
                            lr=3e-3, betas=(0.9, 0.999), eps=1e-8)
    state = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
    hyper = [(3e-3, 0.05), (3e-3, 0.05), (1e-4, 0.0)]
    for step in range(1, 4):
        grads = [K.adamw_inputs(n, i)[1][step - 1].double() for i, n in enumerate(sizes)]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        norm = math.sqrt(R.grad_sumsq(grads))
        clip = R.clip_coef(norm, max_norm)
        if max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
            assert abs(float(total) - norm) <= 1e-12 * norm
            assert (clip == 1.0) == (norm < max_norm)
            _eq(ps[0].grad, grads[0] * clip)
        opt.step()
        state = [R.adamw_step(p, g, m, v, step, lr, (0.9, 0.999), 1e-8, wd, clip)
                 for (p, m, v), g, (lr, wd) in zip(state, grads, hyper)]
        for p, (rp, rm, rv) in zip(ps, state):
            _eq(rp, p.detach(), 1e-13)
            _eq(rm, opt.state[p]["exp_avg"], 1e-13)
            _eq(rv, opt.state[p]["exp_avg_sq"], 1e-13)


# ---- the yardsticks the GPU tests scale their bounds from stay inside the tolerances the suite already uses ----------------
@pytest.mark.parametrize("case", K.BN_SMALL[1:])
def test_bn_fp32_yardstick_within_existing_tolerances(case):
    n, c, hw, _ = case
    d = K.bn_inputs(n, c, hw)
    ref = R.bn_train_forward(d["x"], d["gamma"], d["beta"], d["res"], d["rm"], d["rv"])
    yd = K.bn_forward_yardstick(d, True, True, True)
    for k in ("y", "running_mean", "running_var"):
        assert K.max_err(yd[k], ref[k]) <= FWD(ref[k]), k
    rb = R.bn_train_backward(d["dy"], d["x"], d["gamma"], ref["y"])
    yb = K.bn_backward_yardstick(d, ref["y"], yd)
    for k in ("dx", "dres", "dgamma", "dbeta"):
        assert K.max_err(yb[k], rb[k]) <= K.GRAD_TOL * max(1.0, float(rb[k].abs().max())), k


def FWD(ref):
    return K.FWD_TOL * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("pixels,rows", K.NHWC_PIXELS)
@pytest.mark.parametrize("c,cs", K.NHWC_CH)
def test_bf16_rounding_of_the_fp32_yardstick_stays_inside_the_allowance(pixels, rows, c, cs):
    d = K.nhwc_bwd_inputs(pixels, c, cs)
    for keep in (None, d["y"] > 0):
        ref = R.nhwc_bn_backward(d["gy"], d["x"], d["mean"], d["rstd"], d["gamma"], c, keep)
        yd = K.nhwc_bwd_yardstick(d, c, keep)
        share, steps = K.bf16_mismatch(yd["gx"], ref["gx"])
        assert steps <= 1 and share <= K.BF16_ULP_SHARE, (share, steps)
        assert K.bf16_mismatch(yd["gres"], ref["gres"]) == (0.0, 0)
        for k in ("dgamma", "dbeta"):
            assert K.max_err(yd[k], ref[k]) <= K.GRAD_TOL * max(1.0, float(ref[k].abs().max())), k


@pytest.mark.parametrize("rows", K.FIN_ROWS)
def test_finalize_yardstick_within_existing_tolerances(rows):
    for c, cs in K.FIN_CH:
        d = K.finalize_inputs(rows, c, cs)
        ref = R.nhwc_bn_finalize(d["part"], c, d["count"], d["gamma"], d["beta"], d["rm"], d["rv"])
        yd = K.finalize_yardstick(d, c)
        for k, v in yd.items():
            assert K.max_err(v, ref[k]) <= FWD(ref[k]), (k, c)
