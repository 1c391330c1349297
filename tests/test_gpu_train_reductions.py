"""The reduction kernels of the training step against float64 (tests/reductions_ref.py) at the smallest sizes that reach
every host-side split rule and every loop of theirs: BatchNorm statistics and gradients with 1, 2 and 16 slices per channel, a
second block of the finish kernels, the 64-element flush and the strided apply kernels, channel slices; the bf16 NHWC finalize /
backward / channel sum below, at and above the 385 rows their unrolled loop needs; the three heat-map losses with B and J past
the 256 threads of their finish kernels; the gradient norm and AdamW past their grid-stride thresholds.

Bounds (tests/reductions_cases.py): 4 x the error of torch's fp32 CPU kernels on the same operands, at least 4 ulp of the
reference's maximum, never above the tolerances of tests/test_gpu_train_ops.py; bf16 outputs equal the bf16 rounding of the
float64 result except for one step on at most 1e-3 of the elements; the squared gradient norm to 4 * 2^-24; the AdamW moments
to 2^-24 beta / (1 - beta) + 8 * 2^-24 of the tensor's maximum (the kernel forms 1 - beta from the float beta).  Every test
prints ``REDUCTIONS|case|output|yardstick|kernel error|bound``; profiles/reductions_vs_fp64.txt is that table from an MI355X."""
import ctypes
import functools
import math

import pytest
import torch

from tests import reductions_cases as K
from tests import reductions_ref as R

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2


def _record(case, name, yard, err, bnd):
    print(f"REDUCTIONS|{case}|{name}|{yard:.3e}|{err:.3e}|{bnd:.3e}")


def _check(case, name, out, ref, yard_out, cap):
    yard = 0.0 if yard_out is None else K.max_err(yard_out, ref)
    assert yard <= cap * max(1.0, float(ref.abs().max())), f"{case} {name}: the fp32 yardstick itself is off by {yard}"
    err, bnd = K.max_err(out, ref), K.bound(yard, ref, cap)
    _record(case, name, yard, err, bnd)
    assert err <= bnd, f"{case} {name}: max abs err {err} > {bnd} (fp32 yardstick {yard}, ref max {float(ref.abs().max())})"


# ---- BatchNorm fp32 ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _bn_inputs(n, c, hw):
    return K.bn_inputs(n, c, hw)


def _slices(n, c, hw):
    from otpose_amd import hip
    return hip.lib().otp_bn_workspace(n, c, hw) // (16 * c)


def _bn_compare(case, d, out, relu, with_res, with_running, chunk):
    """``out``: the kernels' y, dx, dres, dgamma, dbeta, running_mean, running_var (+ mean, rstd) on the CPU.  Reference and
    yardstick are evaluated ``chunk`` channels at a time (the operation is independent per channel); errors, yardsticks and
    reference maxima are folded over the chunks before the bound is formed."""
    n, c = d["x"].shape[:2]
    single = n * d["x"].shape[2] == 1
    acc = {}
    for c0 in range(0, c, chunk):
        sl = slice(c0, min(c, c0 + chunk))
        dd = {k: (v[:, sl] if v.dim() == 4 else v[sl]) for k, v in d.items()}
        f = R.bn_train_forward(dd["x"], dd["gamma"], dd["beta"], dd["res"] if with_res else None,
                               dd["rm"] if with_running else None, dd["rv"] if with_running else None, 0.1, 1e-5, relu)
        y_kernel = out["y"][:, sl]
        b = R.bn_train_backward(dd["dy"], dd["x"], dd["gamma"], y_kernel if relu else None)
        if single:                         # torch refuses one value per channel: the bound is its floor, 4 ulp
            yf, yb = {}, {}
        else:
            yf = K.bn_forward_yardstick(dd, relu, with_res, with_running)
            yb = K.bn_backward_yardstick(dd, y_kernel if relu else None, yf)
        f.update(b)
        yf.update(yb)
        for k, ref in f.items():
            if ref is None or k not in out or out[k] is None:
                continue
            o = out[k][:, sl] if out[k].dim() == 4 else out[k][sl]
            e, yd, rmax = K.max_err(o, ref), (K.max_err(yf[k], ref) if k in yf else 0.0), float(ref.abs().max())
            pe, py, pm = acc.get(k, (0.0, 0.0, 0.0))
            acc[k] = (max(pe, e), max(py, yd), max(pm, rmax))
    for k, (e, yd, rmax) in acc.items():
        cap = K.FWD_TOL if k in ("y", "mean", "rstd", "running_mean", "running_var", "dres") else K.GRAD_TOL
        assert yd <= cap * max(1.0, rmax), f"{case} {k}: the fp32 yardstick itself is off by {yd}"
        bnd = K.bound(yd, torch.tensor([rmax]), cap)
        _record(case, k, yd, e, bnd)
        assert e <= bnd, f"{case} {k}: max abs err {e} > {bnd} (fp32 yardstick {yd}, ref max {rmax})"
    need = {"y", "dx", "dgamma", "dbeta"} | ({"dres"} if with_res else set()) | ({"running_mean", "running_var"} if with_running else set())
    assert need <= set(acc), sorted(need - set(acc))


def _bn_through_wrapper(n, c, hw, relu, with_res, with_running):
    from otpose_amd import train_ops as T
    d = _bn_inputs(n, c, hw)
    xs, gs, bs = (d[k].cuda().requires_grad_() for k in ("x", "gamma", "beta"))
    rs = d["res"].cuda().requires_grad_() if with_res else None
    rm, rv = (d["rm"].cuda(), d["rv"].cuda()) if with_running else (None, None)
    y = T.batch_norm_relu(xs, gs, bs, rs, rm, rv, 0.1, 1e-5, relu)
    y.backward(d["dy"].cuda())
    cpu = lambda t: None if t is None else t.detach().cpu()                            # noqa: E731
    return d, {"y": cpu(y), "dx": cpu(xs.grad), "dres": cpu(rs.grad) if with_res else None, "dgamma": cpu(gs.grad),
               "dbeta": cpu(bs.grad), "running_mean": cpu(rm), "running_var": cpu(rv)}


@pytest.mark.parametrize("with_running", [True, False])
@pytest.mark.parametrize("relu,with_res", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("case", K.BN_SMALL)
def test_batch_norm_train_vs_fp64(case, relu, with_res, with_running):
    n, c, hw, s = case
    assert _slices(n, c, hw) == s
    d, out = _bn_through_wrapper(n, c, hw, relu, with_res, with_running)
    _bn_compare(f"bn{case[:3]} relu={int(relu)} res={int(with_res)} run={int(with_running)}", d, out, relu, with_res,
                with_running, c)


def test_batch_norm_train_vs_fp64_strided_apply_and_flush():
    """2048 channels of 16700 values: one slice per channel, 65 or 66 values per thread of the sums (the 64-value flush into
    fp64 happens), and 34 M elements, more than the 16384 x 256 threads of the apply kernels (their stride loop runs)."""
    n, c, hw, s = K.BN_LARGE
    assert _slices(n, c, hw) == s and hw > 64 * 256 and n * c * hw > 16384 * 256
    d, out = _bn_through_wrapper(n, c, hw, True, True, True)
    _bn_compare(f"bn{K.BN_LARGE[:3]} relu=1 res=1 run=1", d, out, True, True, True, 256)


def test_batch_norm_train_channel_slices_vs_fp64():
    """x, res, y (forward) and dy, x, y (backward) as channel slices of wider tensors, through the C entry points the wrapper
    calls; the channels outside the slice keep their bits."""
    from otpose_amd import hip
    n, c, hw, s = 2, 5, 4608, 2
    assert _slices(n, c, hw) == s
    d = _bn_inputs(n, c, hw)
    L = hip.lib()
    wide = lambda ctot, seed: torch.randn(n, ctot, hw, 1, generator=K.gen(seed)).cuda()      # noqa: E731
    (xt, xo), (rt, ro), (yt, yo), (dt, do) = (9, 3), (7, 1), (11, 6), (8, 2)
    xw, rw, yw, dw = wide(xt, 1), wide(rt, 2), wide(yt, 3), wide(dt, 4)
    xw[:, xo:xo + c], rw[:, ro:ro + c], dw[:, do:do + c] = d["x"].cuda(), d["res"].cuda(), d["dy"].cuda()
    before = [t.clone() for t in (xw, rw, yw, dw)]
    gamma, beta, rm, rv = (d[k].cuda() for k in ("gamma", "beta", "rm", "rv"))
    nbytes = L.otp_bn_workspace(n, c, hw)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    mean, rstd, dg, db = (torch.empty(c, device="cuda") for _ in range(4))
    st = hip.stream_of(xw)
    hip.check(L.otp_bn_train_forward(hip.ptr(xw), hip.ptr(gamma), hip.ptr(beta), hip.ptr(rw), hip.ptr(yw), hip.ptr(mean),
                                     hip.ptr(rstd), hip.ptr(rm), hip.ptr(rv), hip.ptr(ws), nbytes, n, c, hw, 1e-5, 0.1, 1,
                                     xt, xo, rt, ro, yt, yo, st), "otp_bn_train_forward")
    dx, dres = torch.empty(n, c, hw, 1, device="cuda"), torch.empty(n, c, hw, 1, device="cuda")
    hip.check(L.otp_bn_train_backward(hip.ptr(dw), hip.ptr(xw), hip.ptr(yw), hip.ptr(mean), hip.ptr(rstd), hip.ptr(gamma),
                                      hip.ptr(dx), hip.ptr(dres), hip.ptr(dg), hip.ptr(db), hip.ptr(ws), nbytes, n, c, hw,
                                      dt, do, xt, xo, yt, yo, st), "otp_bn_train_backward")
    assert torch.equal(xw, before[0]) and torch.equal(rw, before[1]) and torch.equal(dw, before[3])
    assert torch.equal(yw[:, :yo], before[2][:, :yo]) and torch.equal(yw[:, yo + c:], before[2][:, yo + c:])
    cpu = lambda t: t.detach().cpu()                                                   # noqa: E731
    out = {"y": cpu(yw[:, yo:yo + c]), "mean": cpu(mean), "rstd": cpu(rstd), "dx": cpu(dx), "dres": cpu(dres),
           "dgamma": cpu(dg), "dbeta": cpu(db), "running_mean": cpu(rm), "running_var": cpu(rv)}
    _bn_compare("bn(2, 5, 4608) channel slices", d, out, True, True, True, c)


@pytest.mark.parametrize("case", [K.BN_SMALL[1], K.BN_SMALL[2], K.BN_SMALL[3]])
def test_channel_sum_vs_fp64(case):
    from otpose_amd import hip, train_ops as T
    n, c, hw, s = case
    assert _slices(n, c, hw) == s
    a = _bn_inputs(n, c, hw)["dy"]
    ref = R.channel_sum(a)
    _check(f"channel_sum{case[:3]}", "sum", T.channel_sum(a.cuda()), ref, a.sum(dim=(0, 2, 3)), K.GRAD_TOL)
    # the same channels as a slice of a wider tensor
    L = hip.lib()
    ctot, coff = c + 5, 2
    wide = torch.randn(n, ctot, hw, 1, generator=K.gen(9)).cuda()
    wide[:, coff:coff + c] = a.cuda()
    nbytes = L.otp_bn_workspace(n, c, hw) + 4 * c
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device="cuda")
    out = torch.empty(c, device="cuda")
    hip.check(L.otp_channel_sum(hip.ptr(wide), hip.ptr(out), hip.ptr(ws), nbytes, n, c, hw, ctot, coff, hip.stream_of(wide)),
              "otp_channel_sum")
    _check(f"channel_sum{case[:3]} slice", "sum", out, ref, a.sum(dim=(0, 2, 3)), K.GRAD_TOL)


# ---- bf16 NHWC finalize / backward / channel sum -----------------------------------------------------------------------------
@pytest.mark.parametrize("c,cs", K.FIN_CH)
@pytest.mark.parametrize("rows", K.FIN_ROWS)
def test_nhwc_bn_finalize_vs_fp64(rows, c, cs):
    from otpose_amd import bf16_ops as B
    d = K.finalize_inputs(rows, c, cs)
    ref = R.nhwc_bn_finalize(d["part"], c, d["count"], d["gamma"], d["beta"], d["rm"], d["rv"])
    yd = K.finalize_yardstick(d, c)
    rm, rv = d["rm"].cuda(), d["rv"].cuda()
    vec = B.bn_finalize(d["part"].cuda(), rows, c, d["count"], d["gamma"].cuda(), d["beta"].cuda(), rm, rv, 0.1, 1e-5).cpu()
    case = f"nhwc_finalize rows={rows} C={c}/{cs}"
    for i, k in enumerate(("mean", "rstd", "scale", "shift")):
        _check(case, k, vec[i], ref[k], yd[k], K.FWD_TOL)
    _check(case, "running_mean", rm, ref["running_mean"], yd["running_mean"], K.FWD_TOL)
    _check(case, "running_var", rv, ref["running_var"], yd["running_var"], K.FWD_TOL)
    assert float(vec[2, c:].abs().max() if cs > c else 0) == 0 and float(vec[3, c:].abs().max() if cs > c else 0) == 0
    if rows == 129:                       # without running statistics: same vectors
        vec2 = B.bn_finalize(d["part"].cuda(), rows, c, d["count"], d["gamma"].cuda(), d["beta"].cuda(), None, None, 0.1, 1e-5)
        assert torch.equal(vec2.cpu(), vec)


def _bwd_rows(pixels, cs):
    from otpose_amd import hip
    return (hip.lib().otp_nhwc_bn_backward_workspace(pixels, cs) // (4 * cs) - 3) // 2


@pytest.mark.parametrize("relu", [0, 1, 2])
@pytest.mark.parametrize("c,cs", K.NHWC_CH)
@pytest.mark.parametrize("pixels,rows", K.NHWC_PIXELS)
def test_nhwc_bn_backward_vs_fp64(pixels, rows, c, cs, relu):
    """relu: 0 none, 1 the mask is y > 0 of the bf16 y, 2 the mask is the forward's bit mask (one bit per element)."""
    from otpose_amd import bf16_ops as B
    assert _bwd_rows(pixels, cs) == rows
    d = K.nhwc_bwd_inputs(pixels, c, cs)
    keep = d["y"] > 0 if relu else None
    ref = R.nhwc_bn_backward(d["gy"], d["x"], d["mean"], d["rstd"], d["gamma"], c, keep)
    yd = K.nhwc_bwd_yardstick(d, c, keep)
    if relu == 2:
        bits = (keep.reshape(pixels, cs // 8, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(2)
        y = bits.to(torch.uint8).reshape(-1).cuda()
    else:
        y = d["y"].cuda()
    gx, gres, dg, db = B.bn_backward(d["gy"].cuda(), y, d["x"].cuda(), d["mean"].cuda(), d["rstd"].cuda(), d["gamma"].cuda(), c,
                                     bool(relu), True)
    case = f"nhwc_bn_backward pixels={pixels} rows={rows} C={c}/{cs} relu={relu}"
    _check(case, "dgamma", dg, ref["dgamma"], yd["dgamma"], K.GRAD_TOL)
    _check(case, "dbeta", db, ref["dbeta"], yd["dbeta"], K.GRAD_TOL)
    for k, o in (("gx", gx), ("gres", gres)):
        yshare, ysteps = K.bf16_mismatch(yd[k], ref[k])
        share, steps = K.bf16_mismatch(o, ref[k])
        print(f"REDUCTIONS|{case}|{k} bf16 mismatch share (steps)|{yshare:.3e} ({ysteps})|{share:.3e} ({steps})|{K.BF16_ULP_SHARE:.0e} (1)")
        assert ysteps <= 1 and yshare <= K.BF16_ULP_SHARE
        assert steps <= 1 and share <= K.BF16_ULP_SHARE, f"{case} {k}: {share} of the elements differ, by up to {steps} bf16 steps"
    assert float(gx[:, c:].float().abs().max() if cs > c else 0) == 0


@pytest.mark.parametrize("c,cs", K.NHWC_CH)
@pytest.mark.parametrize("pixels,rows", K.NHWC_PIXELS)
def test_nhwc_channel_sum_vs_fp64(pixels, rows, c, cs):
    from otpose_amd import bf16_ops as B, hip
    assert hip.lib().otp_nhwc_channel_sum_workspace(pixels, cs) // (4 * cs) == rows
    g = K.nhwc_bwd_inputs(pixels, c, cs)["gy"]
    ref = g.double().sum(0)[:c]
    _check(f"nhwc_channel_sum pixels={pixels} rows={rows} C={c}/{cs}", "sum", B.channel_sum_nhwc(g.cuda(), c), ref,
           g.float().sum(0)[:c], K.GRAD_TOL)


# ---- losses ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _loss_inputs(b, j, hw):
    return K.loss_inputs(b, j, hw)


def _st_ohkw_direct(d, topk, flags):
    """otp_loss_st_ohkw_grads the way ops.st_ohkw_loss calls otp_loss_st_ohkw, with the third gradient."""
    from otpose_amd import hip
    s, t, g = (d[k].cuda() for k in ("s", "t", "g"))
    b, j, hw = s.shape[:3]
    w = d["w"].reshape(b, j).cuda()
    L = hip.lib()
    nbytes = L.otp_loss_workspace(b, j)
    ws = torch.empty(nbytes // 4, device="cuda")
    res = torch.empty(3, device="cuda")
    fl = flags.to(torch.int32).cuda() if flags is not None else torch.empty(j, dtype=torch.int32, device="cuda")
    gs, gt, gg = torch.empty_like(s), torch.empty_like(t), torch.empty_like(g)
    rc = L.otp_loss_st_ohkw_grads(hip.ptr(s), hip.ptr(t), hip.ptr(g), hip.ptr(w), hip.ptr(fl), hip.ptr(res), hip.ptr(gs),
                                  hip.ptr(gt), hip.ptr(gg), hip.ptr(ws), nbytes, b, j, hw, topk, int(flags is not None),
                                  hip.stream_of(s))
    hip.check(rc, "otp_loss_st_ohkw_grads")
    return {"ohkm_loss_s": res[0], "mse_loss_s": res[1], "final_loss": res[2], "flags": fl, "grad_s": gs, "grad_t": gt,
            "grad_g": gg}


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("case", K.LOSS_CASES)
def test_st_ohkw_loss_vs_fp64(case, given):
    """All three scalars, the flags and all three gradients.  B = 300 and J = 257 / 300 exceed the 256 threads of
    loss_finish_kernel: its per-sample and per-joint terms are strided loops, J is limited only by the 64 KB of LDS."""
    from otpose_amd import ops
    b, j, hw, topk = case
    d = _loss_inputs(b, j, hw)
    flags = torch.roll(d["expected_flags"], 1) if given else None
    ref = R.st_ohkw(d["s"], d["t"], d["g"], d["w"], topk, flags)
    assert R.topk_gap(ref["per_sample"], topk) > K.TOPK_GAP
    assert int((d["w"] == 0).sum()) > 0 or b * j < 8
    yd = K.st_ohkw_yardstick(d, topk, ref["flags"])
    out = _st_ohkw_direct(d, topk, flags)
    assert out["flags"].cpu().tolist() == ref["flags"].tolist()
    if not given:
        assert ref["flags"].tolist() == d["expected_flags"].tolist() and 0 < int(ref["flags"].sum()) < j     # mixed
    name = f"st_ohkw{case} flags={'given' if given else 'derived'}"
    for k in ("ohkm_loss_s", "mse_loss_s", "final_loss"):
        _check(name, k, out[k].reshape(()), ref[k].reshape(()), yd[k].reshape(()), K.FWD_TOL)
    for k in ("grad_s", "grad_t", "grad_g"):
        _check(name, k, out[k], ref[k], yd[k], K.GRAD_TOL)
    w = ops.st_ohkw_loss(d["s"].cuda(), d["t"].cuda(), d["g"].cuda(), d["w"].cuda(), topk, None if flags is None else flags.cuda(),
                         with_grad=True)
    for k in ("ohkm_loss_s", "mse_loss_s", "final_loss", "grad_s", "grad_t", "flags"):
        assert torch.equal(w[k], out[k]), k


@pytest.mark.parametrize("use_w,eff", [(True, None), (True, 13), (False, None), (False, 13)])
@pytest.mark.parametrize("case", K.LOSS_CASES)
def test_joints_losses_vs_fp64(case, use_w, eff):
    from otpose_amd import ops
    b, j, hw, topk = case
    d = _loss_inputs(b, j, hw)
    w = d["w"] if use_w else None
    assert R.topk_gap(R.joints_per_sample(d["s"], d["g"], w), topk) > K.TOPK_GAP
    ref = R.joints_ohkm_mse(d["s"], d["g"], w, eff, topk)
    pv, pg = R.joint_mse(d["s"], d["g"], w, eff)
    yd = K.joints_yardstick(d, topk, use_w, eff)
    wg = None if w is None else w.cuda()
    out = ops.joints_ohkm_mse_loss(d["s"].cuda(), d["g"].cuda(), wg, effective_num_joints=eff, topk=topk, with_grad=True)
    name = f"joints{case} w={int(use_w)} eff={eff}"
    for k in ("ohkm_loss", "mse_loss", "final_loss"):
        _check(name, k, out[k].reshape(()), ref[k].reshape(()), yd[k].reshape(()), K.FWD_TOL)
    _check(name, "grad_output", out["grad_output"], ref["grad_output"], yd["grad_output"], K.GRAD_TOL)
    v, gv = ops.joint_mse_loss(d["s"].cuda(), d["g"].cuda(), wg, effective_num_joints=eff, with_grad=True)
    _check(name, "plain mse", v.reshape(()), pv.reshape(()), yd["plain"].reshape(()), K.FWD_TOL)
    _check(name, "plain mse grad", gv, pg, yd["plain_grad"], K.GRAD_TOL)


# ---- gradient norm and AdamW ---------------------------------------------------------------------------------------------------
LR, BETAS, EPS = 3e-3, (0.9, 0.999), 1e-8


def _adamw_run(name, sizes, hyper, mode, steps=3, preset=None):
    """``sizes``: one single-tensor group each; ``hyper``: (lr, weight_decay) per group; ``mode``: 'off' (max_norm = 0),
    'active' (max_norm = half the smallest norm of the steps) or 'inactive' (twice the largest: the coefficient is exactly 1).
    ``preset``: (step, seed) - moments and step count loaded through load_state_dict first."""
    from otpose_amd.optim import FusedAdamW
    data = [K.adamw_inputs(n, i) for i, n in enumerate(sizes)]
    norms = [math.sqrt(R.grad_sumsq([gs[it] for _, gs in data])) for it in range(steps)]
    max_norm = {"off": 0.0, "active": 0.5 * min(norms), "inactive": 2.0 * max(norms)}[mode]
    params = [torch.nn.Parameter(p0.cuda()) for p0, _ in data]
    opt = FusedAdamW([{"params": [p], "lr": lr, "weight_decay": wd} for p, (lr, wd) in zip(params, hyper)], lr=LR, betas=BETAS,
                     eps=EPS, max_grad_norm=max_norm)
    state = [(p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
             for (p0, _), n in zip(data, sizes)]
    step0 = 0
    if preset is not None:
        step0, seed = preset
        g = K.gen(seed)
        moments = [(0.05 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g)) for n in sizes]
        sd = opt.state_dict()
        for i, (m, v) in enumerate(moments):
            sd["state"][i] = {"step": step0, "exp_avg": m.cuda(), "exp_avg_sq": v.cuda()}
        opt.load_state_dict(sd)
        state = [(p, m.double(), v.double()) for (p, _, _), (m, v) in zip(state, moments)]
    worst = {"normsq": 0.0, "p": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    for it in range(steps):
        opt.zero_grad()
        for p, (_, gs) in zip(params, data):
            p.grad = gs[it].cuda()                             # an ordinary tensor: step() copies it into the flat slot
        ref_sq = R.grad_sumsq([gs[it] for _, gs in data])
        got_sq = float(opt.grad_norm()) ** 2
        worst["normsq"] = max(worst["normsq"], abs(got_sq - ref_sq) / ref_sq)
        assert abs(got_sq - ref_sq) <= K.SUMSQ_RTOL * ref_sq, (name, it, got_sq, ref_sq)
        clip = R.clip_coef(math.sqrt(ref_sq), max_norm)
        assert {"off": clip == 1.0, "active": clip < 1.0, "inactive": clip == 1.0}[mode]
        opt.step()
        state = [R.adamw_step(p, gs[it], m, v, step0 + it + 1, lr, BETAS, EPS, wd, clip)
                 for (p, m, v), (_, gs), (lr, wd) in zip(state, data, hyper)]
        for p, (rp, rm, rv) in zip(params, state):
            for key, out, ref, rtol in (("p", p, rp, None), ("exp_avg", opt.state[p]["exp_avg"], rm, K.moment_rtol(BETAS[0])),
                                        ("exp_avg_sq", opt.state[p]["exp_avg_sq"], rv, K.moment_rtol(BETAS[1]))):
                err, rmax = K.max_err(out, ref), float(ref.abs().max())
                scale = max(1.0, rmax) if rtol is None else rmax
                bnd = (K.P_TOL if rtol is None else rtol) * scale
                worst[key] = max(worst[key], err / scale)
                assert err <= bnd, f"{name} step {it} {key}: max abs err {err} > {bnd} (ref max {rmax})"
    print(f"REDUCTIONS|{name} clip={mode}|normsq rel err|-|{worst['normsq']:.3e}|{K.SUMSQ_RTOL:.3e}")
    print(f"REDUCTIONS|{name} clip={mode}|p err / max(1, max|p|)|-|{worst['p']:.3e}|{K.P_TOL:.3e}")
    for key, beta in (("exp_avg", BETAS[0]), ("exp_avg_sq", BETAS[1])):
        print(f"REDUCTIONS|{name} clip={mode}|{key} err / max|-|{worst[key]:.3e}|{K.moment_rtol(beta):.3e}")


@pytest.mark.parametrize("mode", ["off", "active", "inactive"])
@pytest.mark.parametrize("n", K.ADAMW_SIZES)
def test_fused_adamw_single_group_vs_fp64(n, mode):
    """n < 4: no float4 body; 1 310 723 and 4 200 003: past the grid strides of the sum of squares (1024 x 256 x 4) and of the
    update (4096 x 256 x 4), each with an n % 4 tail."""
    _adamw_run(f"adamw n={n}", [n], [(LR, 0.05)], mode)


@pytest.mark.parametrize("mode", ["off", "active", "inactive"])
def test_fused_adamw_three_groups_vs_fp64(mode):
    """The squared norm accumulates across the groups' launches (``*acc +=``), every group with a tail."""
    _adamw_run("adamw groups=(1310723, 4200003, 5)", [1310723, 4200003, 5], [(LR / 100, 0.05), (LR, 0.05), (LR, 0.0)], mode)


def test_fused_adamw_resumed_at_step_1000_vs_fp64():
    _adamw_run("adamw n=1027 from step 1000", [1027], [(LR, 0.05)], "active", steps=2, preset=(1000, 77))


def test_optimizer_entry_points_refuse_unaligned_pointers():
    """A pointer that is not 16-byte aligned: OTP_ERR_UNSUPPORTED, and nothing is written."""
    from otpose_amd import hip
    L = hip.lib()
    n = 1023
    p, g, m, v = (torch.randn(n + 1, generator=K.gen(i)).cuda() for i in range(4))
    acc = torch.full((1 + int(L.otp_grad_sumsq_scratch()),), 3.0, dtype=torch.float64, device="cuda")
    before = [t.clone() for t in (p, g, m, v, acc)]
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)                                     # noqa: E731
    st = hip.stream_of(p)
    assert L.otp_grad_sumsq(off(g), n, hip.ptr(acc), st) == UNSUPPORTED
    for args in ((off(p), hip.ptr(g), hip.ptr(m), hip.ptr(v)), (hip.ptr(p), off(g), hip.ptr(m), hip.ptr(v)),
                 (hip.ptr(p), hip.ptr(g), off(m), hip.ptr(v)), (hip.ptr(p), hip.ptr(g), hip.ptr(m), off(v))):
        assert L.otp_adamw_step(*args, n, LR, 0.9, 0.999, EPS, 0.05, 1, hip.ptr(acc), 1.0, st) == UNSUPPORTED
    torch.cuda.synchronize()
    for t, b in zip((p, g, m, v, acc), before):
        assert torch.equal(t, b)
