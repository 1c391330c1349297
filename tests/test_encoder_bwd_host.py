"""tests/encoder_bwd_ref.py and tests/encoder_bwd_cases.py pinned on the CPU: every float64 restatement against torch's float64
autograd of the same expression (1e-12), every case's fp32 yardstick inside its cap, and the branch each case is named for
derived again from the case's numbers by the host rule it restates - so that tests/test_gpu_encoder_bwd.py keeps reaching every
branch and loop it was written for."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import encoder_bwd_cases as C
from tests import encoder_bwd_ref as E
from tests import reductions_cases as K

D = torch.float64


def _eq(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _within_cap(name, yard, ref, cap):
    err = K.max_err(yard, ref)
    assert err <= cap * max(1.0, float(ref.abs().max())), f"{name}: the fp32 yardstick is off by {err}"
    return err


# ---- restatements vs float64 autograd ------------------------------------------------------------------------------------
def test_layer_norm_restatement():
    d = {k: v.double() for k, v in C.ln_inputs(2, 7, 9).items()}
    r = E.layer_norm(d["x"], d["gamma"], d["beta"], d["dy"])
    y, (dx, dg, db) = E._autograd(E.layer_norm_expr, [d["x"], d["gamma"], d["beta"]], d["dy"])
    _eq(r["y"], y)
    _eq(r["dx"], dx)
    _eq(r["dgamma"], dg.reshape(-1))
    _eq(r["dbeta"], db.reshape(-1))
    yd = E.layer_norm_yardstick(d["x"], d["gamma"], d["beta"], d["dy"])              # the same code in float64
    _eq(r["dyxh"], yd["dyxh"])


@pytest.mark.parametrize("t,stride", [(1, 1), (1, 2), (2, 1), (2, 2), (8, 1), (9, 2), (10, 2), (11, 3)])
def test_dwconv3_restatement(t, stride):
    d = {k: v.double() for k, v in C.dwconv_inputs(2, 3, t, stride).items()}
    r = E.dwconv3(d["x"], d["w"], d["dy"], stride)
    y, (dx, dw) = E._autograd(lambda a, k: F.conv1d(a, k, None, stride, 1, 1, 3), [d["x"], d["w"]], d["dy"])
    _eq(r["y"], y)
    _eq(r["dx"], dx)
    _eq(r["dw"], dw)
    _eq(E.dwconv3(d["x"], d["w"], d["dy"], stride, d["prefill"])["dw"], d["prefill"] + dw)


@pytest.mark.parametrize("c,heads,t", [(10, 2, 7), (5, 1, 3)])
def test_chan_attn_restatement(c, heads, t):
    d = {k: v.double() for k, v in C.attn_inputs(2, c, t).items()}
    scale = 1.0 / math.sqrt(c // heads)
    r = E.chan_attn(d["q"], d["k"], d["v"], heads, scale, d["go"])
    out, (dq, dk, dv) = E._autograd(lambda a, b, c_: E.chan_attn_expr(a, b, c_, heads, scale), [d["q"], d["k"], d["v"]], d["go"])
    for name, ref in (("out", out), ("dq", dq), ("dk", dk), ("dv", dv)):
        _eq(r[name], ref)


def test_softmax_backward_restatement():
    d = C.softmax_inputs(5, 3)
    hs, hsp = 5, d["hsp"]
    assert hsp == 16
    _eq(d["p"][:, :hs].sum(-1), torch.ones(C.SOFTMAX_BH, hs), 1e-6)
    r = E.softmax_backward_padded(d["slabs"], d["p"], hs)
    s = torch.randn(C.SOFTMAX_BH, hs, hs, dtype=D, generator=K.gen(1)).requires_grad_()
    p = torch.softmax(s, -1)
    dp = d["slabs"].double().sum(1)[:, :hs, :hs]
    (ds,) = torch.autograd.grad(p, s, dp)
    _eq(E.softmax_backward(dp, p.detach()), ds)
    _eq(r["dS"][:, :hs, :hs], E.softmax_backward(dp, d["p"][:, :hs, :hs]))
    for k in ("dS", "dST", "PT"):
        pad = r[k].clone()
        pad[:, :hs, :hs] = 0
        assert r[k].shape == (C.SOFTMAX_BH, hsp, hsp) and float(pad.abs().max()) == 0.0
    assert torch.equal(r["dST"], r["dS"].transpose(1, 2)) and torch.equal(r["PT"], d["p"].double().transpose(1, 2))


@pytest.mark.parametrize("t", [1, 2, 3, 77, 96])
def test_maxpool_restatement_and_first_maximum_rule(t):
    """Integer inputs with ties: the explicit loop and torch's CPU max_pool1d backward pick the same element."""
    d = C.pool_inputs(t)
    x = d["x"]
    assert float(x[0].min()) == float(x[0].max()) and (t == 1 or bool((x[1, 1:] < x[1, :-1]).all()))
    if t >= 77:
        w = F.pad(x[2:], (1, 1), value=-9.0).unfold(1, 3, 2)                           # windows of the random rows
        assert int(((w == w.max(-1, keepdim=True).values).sum(-1) > 1).sum()) > 10     # ties in many of them
    r = E.maxpool3s2(x, d["dy"])
    for yd in (E.maxpool3s2_yardstick(x.double(), d["dy"].double()), E.maxpool3s2_yardstick(x, d["dy"])):
        assert torch.equal(r["y"], yd["y"].double())
        _eq(r["dx"], yd["dx"].double(), 1e-6)
    assert torch.equal(r["dx"], E.maxpool3s2_yardstick(x.double(), d["dy"].double())["dx"])


def test_gelu_restatement():
    x = torch.tensor(C.GELU_SMALL + [-m for m in C.GELU_SMALL], dtype=D)
    dy = torch.randn(x.shape, dtype=D, generator=K.gen(2))
    r = E.gelu(x, dy)
    yd = E.gelu_yardstick(x, dy)
    _eq(r["y"], yd["y"])
    _eq(r["dx"], yd["dx"])
    big = torch.tensor(C.GELU_LARGE, dtype=D)
    r = E.gelu(torch.cat([big, -big]), torch.ones(2 * big.numel(), dtype=D))
    n = big.numel()
    assert torch.equal(r["y"][:n].float(), big.float()) and float(r["y"][n:].abs().max()) < 1e-20
    assert torch.equal(r["dx"][:n], torch.ones(n, dtype=D)) and float(r["dx"][n:].abs().max()) < 1e-20


@pytest.mark.parametrize("f", C.UPLIN_F)
@pytest.mark.parametrize("t", [1, 2, 7])
def test_upsample_linear_restatement(t, f):
    d = {k: v.double() for k, v in C.uplin_inputs(t, f).items()}
    r = E.upsample_linear(d["x"], f, d["dy"])
    yd = E.upsample_linear_yardstick(d["x"], f, d["dy"])
    _eq(r["y"], yd["y"])
    _eq(r["dx"], yd["dx"])


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("case", C.UPADD_CASES[:2])
def test_upsample_add_restatement(case, relu):
    low_shape, f, _ = case
    d = C.upadd_inputs(low_shape, f, relu)
    r = E.upsample_add(d["low"], d["res"], f, relu, d["dy"])
    yd = E.upsample_add_yardstick(d["low"].double(), d["res"].double(), f, relu, d["dy"].double())
    for k in ("y", "dres", "dlow"):
        _eq(r[k], yd[k])


# ---- fp32 yardsticks inside their caps, branches from the numbers ---------------------------------------------------------
@pytest.mark.parametrize("case", C.DWCONV_CASES)
def test_dwconv_case(case):
    b, c, t, stride, offset, branch = case
    assert C.dwconv_branch(b, c, t, stride, offset) == branch
    d = C.dwconv_inputs(b, c, t, stride, offset)
    for k in ("x", "dy"):
        assert d[k].is_contiguous() and d[k].storage_offset() == offset
    for prefill in (None, d["prefill"]):
        ref, yd = E.dwconv3(d["x"], d["w"], d["dy"], stride, prefill), E.dwconv3_yardstick(d["x"], d["w"], d["dy"], stride, prefill)
        _within_cap("y", yd["y"], ref["y"], C.FWD_TOL)
        _within_cap("dx", yd["dx"], ref["dx"], C.FWD_TOL)
        _within_cap("dw", yd["dw"], ref["dw"], C.GRAD_TOL)


def test_dwconv_cases_cover_the_loops():
    """The paired loop with and without idle threads, its tail alone, the scalar branch at both strides, the unaligned view."""
    names = [c[-1] for c in C.DWCONV_CASES]
    assert any("loop=1024" in n and "tail=0" not in n for n in names)
    assert any("loop=" in n and 0 < int(n.split("loop=")[1].split()[0]) < 1024 for n in names)
    assert any("loop=0" in n for n in names) and any("rows=1 " in n for n in names)
    assert {c[3] for c in C.DWCONV_CASES if c[-1] == "scalar"} == {1, 2}
    assert any(c[4] % 4 and c[2] % 4 == 0 and c[3] == 1 for c in C.DWCONV_CASES)


@functools.lru_cache(maxsize=None)
def _ln_yard_errors(b, c, t, m):
    d = C.ln_inputs(b, c, t, m)
    ref = E.layer_norm(d["x"], d["gamma"], d["beta"], d["dy"])
    yd = E.layer_norm_yardstick(d["x"], d["gamma"], d["beta"], d["dy"])
    return {k: (K.max_err(yd[k], ref[k]), C.LN_CAPS[k] * max(1.0, float(ref[k].abs().max()))) for k in C.LN_CAPS}


@pytest.mark.parametrize("case", C.LN_CASES)
def test_layer_norm_case(case):
    b, c, t, m, branch = case
    assert C.ln_branch(c, t) == branch
    for k, (err, cap) in _ln_yard_errors(b, c, t, m).items():
        assert err <= cap, f"{k}: the fp32 yardstick is off by {err} (cap {cap})"


@pytest.mark.parametrize("case", C.LN_DIRECT_CASES)
def test_layer_norm_direct_case(case):
    b, c, t, branch = case
    assert C.ln_branch(c, t, direct=True) == branch
    for k, (err, cap) in _ln_yard_errors(b, c, t, 0).items():
        assert err <= cap, f"{k}: the fp32 yardstick is off by {err} (cap {cap})"


def test_layer_norm_offset_is_the_largest_the_yardstick_passes():
    (case,) = [c for c in C.LN_CASES if c[3]]
    b, c, t, m, _ = case
    passing = [o for o in C.LN_OFFSETS if all(e <= cap for e, cap in _ln_yard_errors(b, c, t, o).values())]
    assert m == max(passing), (m, passing)


def test_layer_norm_cases_cover_the_kernels():
    names = [c[-1] for c in C.LN_CASES] + [c[-1] for c in C.LN_DIRECT_CASES]
    for kind in ("split-sums", "split-dyxh", "wide", "generic"):
        assert any(n.startswith(kind + " ") for n in names), kind
    assert any(n.startswith("generic") and "tiles=2" in n for n in names)
    assert any(n.startswith("wide") and "last=256" in n for n in names) and any(n.startswith("wide") and "last=4" in n for n in names)
    assert any("empty=3" in n for n in names) and any("empty=2" in n for n in names)
    # either side of the wide rule
    assert {(c[2] % 4 == 0, c[2] >= 1024) for c in C.LN_CASES if c[1] <= C.LN_SPLIT_MAX_C} >= {(True, False), (False, False), (True, True)}


@pytest.mark.parametrize("case", C.ATTN_CASES)
def test_attention_case(case):
    b, c, heads, t, mag, branch = case
    assert C.attn_branch(b, c, heads, t) == branch
    d = C.attn_inputs(b, c, t, mag)
    scale = 1.0 / math.sqrt(c // heads)
    ref = E.chan_attn(d["q"], d["k"], d["v"], heads, scale, d["go"])
    yd = E.chan_attn_yardstick(d["q"], d["k"], d["v"], heads, scale, d["go"])
    for k in ("out", "dq", "dk", "dv"):
        _within_cap(k, yd[k], ref[k], C.ATTN_TOL)
        assert 4 * K.max_err(yd[k], ref[k]) <= C.ATTN_TOL * float(ref[k].abs().max())      # the 2e-4 floor decides the bound


def test_attention_cases_cover_the_branches():
    wide = [c for c in C.ATTN_CASES if c[1] // c[2] > C.WIDE_HEAD]
    assert any("splits=1" in c[-1] for c in wide) and any("splits=1" not in c[-1] for c in wide)
    assert {c[1] // c[2] for c in C.ATTN_CASES} >= {16, 68, 96, 102, 112}
    assert any("NB=7" in c[-1] and "pad=0" in c[-1] for c in C.ATTN_CASES) and any("NB=6" in c[-1] for c in C.ATTN_CASES)
    assert any(c[4] == 1e-8 and c[1] // c[2] > C.WIDE_HEAD for c in C.ATTN_CASES)


@pytest.mark.parametrize("hs,ns", C.SOFTMAX_CASES)
def test_softmax_backward_case(hs, ns):
    d = C.softmax_inputs(hs, ns)
    ref, yd = E.softmax_backward_padded(d["slabs"], d["p"], hs), E.softmax_backward_padded_yardstick(d["slabs"], d["p"], hs)
    _within_cap("dS", yd["dS"], ref["dS"], C.GRAD_TOL)


def test_softmax_and_transpose_cases_cover_the_edges():
    assert {hs % 16 == 0 for hs, _ in C.SOFTMAX_CASES} == {True, False}
    assert {hs > 64 for hs, _ in C.SOFTMAX_CASES} == {True, False} and max(hs for hs, _ in C.SOFTMAX_CASES) == 112
    assert {ns for _, ns in C.SOFTMAX_CASES} == {1, 3}
    assert any(r % 32 and cc % 32 for _, r, cc in C.TRANSPOSE_CASES) and (1, 32, 32) in C.TRANSPOSE_CASES
    assert any(r == 1 for _, r, _ in C.TRANSPOSE_CASES) and any(r > 32 or cc > 32 for _, r, cc in C.TRANSPOSE_CASES)


def test_gelu_case():
    d = C.gelu_inputs()
    assert C.GELU_N > 8192 * 256 and C.GELU_N % 256
    x = d["x"]
    assert x[:64].tolist() == [s * m for m in map(float, torch.tensor(C.GELU_SMALL + C.GELU_LARGE)) for s in (1.0, -1.0)]
    ref, yd = E.gelu(x, d["dy"]), E.gelu_yardstick(x, d["dy"])
    seen = torch.zeros(C.GELU_N, dtype=torch.bool)
    for name, idx in C.gelu_groups():
        seen[idx] = True
        for k in ("y", "dx"):
            assert bool(torch.isfinite(yd[k][idx]).all())
            _within_cap(f"{name} {k}", yd[k][idx], ref[k][idx], C.FWD_TOL)
    assert bool(seen.all())


@pytest.mark.parametrize("f", C.UPLIN_F)
@pytest.mark.parametrize("t", C.UPLIN_T)
def test_upsample_linear_case(t, f):
    d = C.uplin_inputs(t, f)
    ref, yd = E.upsample_linear(d["x"], f, d["dy"]), E.upsample_linear_yardstick(d["x"], f, d["dy"])
    _within_cap("y", yd["y"], ref["y"], C.FWD_TOL)
    _within_cap("dx", yd["dx"], ref["dx"], C.FWD_TOL)
    ctot, coff = C.UPLIN_SLICE
    assert coff > 0 and coff + C.UPLIN_BC[1] < ctot


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("case", C.UPADD_CASES)
def test_upsample_add_case(case, relu):
    low_shape, f, branch = case
    assert C.upadd_branch(low_shape, f) == branch
    d = C.upadd_inputs(low_shape, f, relu)
    ref, yd = E.upsample_add(d["low"], d["res"], f, relu, d["dy"]), E.upsample_add_yardstick(d["low"], d["res"], f, relu, d["dy"])
    for k in ("y", "dres", "dlow"):
        _within_cap(k, yd[k], ref[k], C.FWD_TOL)
    if relu:
        zeros = d["zero"] & (ref["y"] == 0)
        assert int(zeros.sum()) >= C.UPADD_MIN_ZEROS and bool((d["zero"] <= (ref["y"] == 0)).all())
        assert float(ref["dres"][zeros].abs().max()) == 0.0 and float(yd["dres"][zeros].abs().max()) == 0.0


def test_upsample_add_cases_cover_both_forwards():
    assert {c[2] for c in C.UPADD_CASES} == {"scalar", "vec"} and {c[1] for c in C.UPADD_CASES} == {2, 4, 8}
    assert any(c[0][3] % 2 for c in C.UPADD_CASES)
