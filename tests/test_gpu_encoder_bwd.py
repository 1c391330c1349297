"""The small backward kernels of the temporal encoders (csrc/transformer_bwd.hip, csrc/glue.hip, the attention
products and backward helpers of csrc/chanattn.hip, the products on bfloat16 pieces)
against float64 (tests/encoder_bwd_ref.py) at the smallest sizes that reach every host-side branch rule and every loop of theirs
(tests/encoder_bwd_cases.py names the branch of each case; tests/test_encoder_bwd_host.py derives it again from the numbers):
the depthwise conv's dW in and around its paired float4 loop, into a zero and into a pre-filled destination, and on views that are
not 16-byte aligned; the four LayerNorm backward kernels across tile edges, channel-to-wave splits and the wide rule, with a mean
32 standard deviations off zero; the attention backward at head sizes 16 .. 112 with one to four score slices; the softmax
backward and the scaled transpose on their own, padding and tile edges included; max-pool with ties everywhere; GELU past its
grid cap and in both tails; the linear up-sampling backward from T = 1 and from a channel slice; the fuse rows' up-sample-add
backward with outputs that are exactly zero.

Bounds (tests/encoder_bwd_cases.py): 4 x the error of torch's fp32 CPU autograd on the same operands, at least 4 ulp of the
reference's maximum, never above 3e-5 (forwards, element-wise dx) / 1e-4 (the other gradients) of max(1, max|ref|); attention
gradients max(4 x yardstick, 2e-4 of the gradient's maximum); bit-equality for max-pool, the transposes and the zero padding.
Every test prints ``ENCBWD|case|output|yardstick|kernel error|bound``; profiles/encoder_bwd_vs_fp64.txt is that table from an
MI355X."""
import functools
import math

import pytest
import torch

from tests import encoder_bwd_cases as C
from tests import encoder_bwd_ref as E
from tests import reductions_cases as K

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _record(case, name, yard, err, bnd):
    print(f"ENCBWD|{case}|{name}|{yard:.3e}|{err:.3e}|{bnd:.3e}")


def _check(case, name, out, ref, yard_out, cap, bound=None):
    out = out.detach().cpu()
    assert bool(torch.isfinite(out).all()), f"{case} {name}: inf or NaN"
    yard = K.max_err(yard_out, ref)
    assert yard <= cap * max(1.0, float(ref.abs().max())), f"{case} {name}: the fp32 yardstick itself is off by {yard}"
    err, bnd = K.max_err(out, ref), (bound(yard, ref) if bound else K.bound(yard, ref, cap))
    _record(case, name, yard, err, bnd)
    assert err <= bnd, f"{case} {name}: max abs err {err} > {bnd} (fp32 yardstick {yard}, ref max {float(ref.abs().max())})"


def _check_equal(case, name, out, expect):
    out, expect = out.detach().cpu(), expect.detach().cpu().to(torch.float32)
    assert out.shape == expect.shape, (out.shape, expect.shape)
    assert bool(torch.isfinite(out).all()), f"{case} {name}: inf or NaN"
    _record(case, name, 0.0, float((out.double() - expect.double()).abs().max()) if out.numel() else 0.0, 0.0)
    assert torch.equal(out, expect), f"{case} {name}: not bit-equal"


def _gpu_view(t):
    """``t`` on the GPU with the storage offset it has on the CPU (``.cuda()`` of a view would start a fresh, aligned storage)."""
    off = t.storage_offset()
    buf = torch.zeros(off + t.numel(), dtype=t.dtype, device="cuda")
    buf[off:] = t.reshape(-1).cuda()
    v = buf[off:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


# ---- depthwise conv ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefilled", [False, True])
@pytest.mark.parametrize("case", C.DWCONV_CASES)
def test_dwconv3_vs_fp64(case, prefilled):
    """``prefilled``: the weight gradient lands in a slot that already holds seeded values, the way train_ops.grad_slot hands the
    optimizer's buffer to the accumulating kernel; expected is prefill + dW."""
    from otpose_amd import train_ops as T
    b, c, t, stride, offset, branch = case
    d = C.dwconv_inputs(b, c, t, stride, offset)
    prefill = d["prefill"] if prefilled else None
    ref = E.dwconv3(d["x"], d["w"], d["dy"], stride, prefill)
    yd = E.dwconv3_yardstick(d["x"], d["w"], d["dy"], stride, prefill)
    xs, ws, dy = _gpu_view(d["x"]).requires_grad_(), d["w"].cuda().requires_grad_(), _gpu_view(d["dy"])
    if prefilled:
        slot = d["prefill"].cuda()
        ws._otp_grad_slot, ws._otp_slot_epoch = slot, [1, True]
    y = T.dwconv3(xs, ws, stride)
    y.backward(dy)
    name = f"dwconv{case[:5]} {branch} prefill={int(prefilled)}"
    _check(name, "y", y, ref["y"], yd["y"], C.FWD_TOL)
    _check(name, "dx", xs.grad, ref["dx"], yd["dx"], C.FWD_TOL)
    _check(name, "dw", ws.grad, ref["dw"], yd["dw"], C.GRAD_TOL)
    if prefilled:
        _check(name, "dw slot", slot, ref["dw"], yd["dw"], C.GRAD_TOL)                   # the kernel added to the slot itself


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _ln_reference(b, c, t, m):
    d = C.ln_inputs(b, c, t, m)
    return d, E.layer_norm(d["x"], d["gamma"], d["beta"], d["dy"]), E.layer_norm_yardstick(d["x"], d["gamma"], d["beta"], d["dy"])


@pytest.mark.parametrize("case", C.LN_CASES)
def test_layer_norm_vs_fp64(case):
    from otpose_amd import hip
    from otpose_amd import train_ops as T
    b, c, t, m, branch = case
    assert bool(hip.lib().otp_ln_channel_backward_workspace(b, c, t)) == (not branch.startswith("generic"))
    d, ref, yd = _ln_reference(b, c, t, m)
    xs, gs, bs = (d[k].cuda().requires_grad_() for k in ("x", "gamma", "beta"))
    y = T.layer_norm(xs, gs, bs, 1e-5)
    y.backward(d["dy"].cuda())
    name = f"ln{case[:4]} {branch}"
    _check(name, "y", y, ref["y"], yd["y"], C.LN_CAPS["y"])
    _check(name, "dx", xs.grad, ref["dx"], yd["dx"], C.LN_CAPS["dx"])
    _check(name, "dgamma", gs.grad.reshape(-1), ref["dgamma"], yd["dgamma"], C.LN_CAPS["dgamma"])
    _check(name, "dbeta", bs.grad.reshape(-1), ref["dbeta"], yd["dbeta"], C.LN_CAPS["dbeta"])


@pytest.mark.parametrize("case", C.LN_DIRECT_CASES)
def test_ln_channel_backward_entry_point_vs_fp64(case):
    """otp_ln_channel_backward itself (dx and dy * xhat out): train_ops reaches it only for C > 136, its 64-token kernel for
    narrower tensors is reachable through the C interface alone."""
    from otpose_amd import hip
    b, c, t, branch = case
    d, ref, yd = _ln_reference(b, c, t, 0)
    x, dy, g = d["x"].cuda(), d["dy"].cuda(), d["gamma"].reshape(-1).cuda()
    gx, dyxh = torch.full_like(x, NAN), torch.full_like(x, NAN)
    hip.check(hip.lib().otp_ln_channel_backward(hip.ptr(x), hip.ptr(dy), hip.ptr(g), hip.ptr(gx), hip.ptr(dyxh), b, c, t, 1e-5,
                                                hip.stream_of(x)), "otp_ln_channel_backward")
    name = f"ln-direct{case[:3]} {branch}"
    _check(name, "dx", gx, ref["dx"], yd["dx"], C.LN_CAPS["dx"])
    _check(name, "dyxh", dyxh, ref["dyxh"], yd["dyxh"], C.LN_CAPS["dyxh"])


# ---- attention backward ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _attn_reference(b, c, heads, t, mag):
    d = C.attn_inputs(b, c, t, mag)
    scale = 1.0 / math.sqrt(c // heads)
    return (d, E.chan_attn(d["q"], d["k"], d["v"], heads, scale, d["go"]),
            E.chan_attn_yardstick(d["q"], d["k"], d["v"], heads, scale, d["go"]))


@pytest.mark.parametrize("case", C.ATTN_CASES)
def test_chan_attn_backward_vs_fp64(case):
    from otpose_amd import hip
    from otpose_amd import train_ops as T
    b, c, heads, t, mag, branch = case
    assert hip.lib().otp_chan_attn_splits(b * heads, t) == C.attn_splits(b * heads, t)
    d, ref, yd = _attn_reference(b, c, heads, t, mag)
    leaves = [d[k].cuda().requires_grad_() for k in ("q", "k", "v")]
    out = T.chan_attn(*leaves, heads, 1.0 / math.sqrt(c // heads))
    out.backward(d["go"].cuda())
    name = f"attn{case[:5]} {branch}"
    _check(name, "out", out, ref["out"], yd["out"], C.ATTN_TOL, C.attn_bound)
    for k, leaf in zip(("dq", "dk", "dv"), leaves):
        _check(name, k, leaf.grad, ref[k], yd[k], C.ATTN_TOL, C.attn_bound)


def test_chan_attn_cases_run_with_one_and_with_several_score_slices():
    """Read from the library: of the wide-head cases at least one has a single slice of T and one has more."""
    from otpose_amd import hip
    ns = {hip.lib().otp_chan_attn_splits(b * heads, t) for b, c, heads, t, _, _ in C.ATTN_CASES if c // heads > C.WIDE_HEAD}
    assert 1 in ns and max(ns) > 1, ns


@pytest.mark.parametrize("hs,ns", C.SOFTMAX_CASES)
def test_softmax_backward_vs_fp64(hs, ns):
    from otpose_amd import hip
    d = C.softmax_inputs(hs, ns)
    hsp, bh = d["hsp"], C.SOFTMAX_BH
    ref, yd = E.softmax_backward_padded(d["slabs"], d["p"], hs), E.softmax_backward_padded_yardstick(d["slabs"], d["p"], hs)
    slabs, p = d["slabs"].cuda(), d["p"].cuda()
    d_s, d_st, p_t = (torch.full((bh, hsp, hsp), NAN, device="cuda") for _ in range(3))
    hip.check(hip.lib().otp_softmax_backward(hip.ptr(slabs), hip.ptr(p), hip.ptr(d_s), hip.ptr(d_st), hip.ptr(p_t), bh, hs, ns,
                                             hip.stream_of(p)), "otp_softmax_backward")
    name = f"softmax_bwd(hs={hs}, NS={ns})"
    _check(name, "dS", d_s, ref["dS"], yd["dS"], C.GRAD_TOL)
    _check_equal(name, "dST", d_st, d_s.transpose(1, 2))
    _check_equal(name, "PT", p_t, d["p"].transpose(1, 2))
    pad = d_s.cpu().clone()
    pad[:, :hs, :hs] = 0
    _check_equal(name, "dS padding", pad, torch.zeros(bh, hsp, hsp))


@pytest.mark.parametrize("scale", C.TRANSPOSE_SCALES)
@pytest.mark.parametrize("case", C.TRANSPOSE_CASES)
def test_transpose_scale_bit_equal(case, scale):
    from otpose_amd import hip
    batches, r, cc = case
    x = torch.randn(batches, r, cc, generator=K.gen(7800 + r))
    xs = x.cuda()
    out = torch.full((batches, cc, r), NAN, device="cuda")
    hip.check(hip.lib().otp_transpose_scale(hip.ptr(xs), hip.ptr(out), batches, r, cc, scale, hip.stream_of(xs)),
              "otp_transpose_scale")
    _check_equal(f"transpose{case} scale={scale:.6g}", "out", out, x.transpose(1, 2) * torch.tensor(scale, dtype=torch.float32))


# ---- max-pool, GELU, linear up-sampling ------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", C.POOL_T)
def test_maxpool3s2_ties_bit_equal(t):
    from otpose_amd import train_ops as T
    d = C.pool_inputs(t)
    ref = E.maxpool3s2(d["x"], d["dy"])
    b, c = C.POOL_ROWS
    xs = d["x"].view(b, c, t).cuda().requires_grad_()
    y = T.maxpool3s2(xs)
    y.backward(d["dy"].view(b, c, -1).cuda())
    _check_equal(f"maxpool(T={t})", "y", y.reshape(b * c, -1), ref["y"])
    _check_equal(f"maxpool(T={t})", "dx", xs.grad.reshape(b * c, t), ref["dx"])


def test_gelu_vs_fp64_past_the_grid_cap_and_in_the_tails():
    from otpose_amd import train_ops as T
    d = C.gelu_inputs()
    ref, yd = E.gelu(d["x"], d["dy"]), E.gelu_yardstick(d["x"], d["dy"])
    xs = d["x"].cuda().requires_grad_()
    y = T.gelu(xs)
    y.backward(d["dy"].cuda())
    out = {"y": y.detach().cpu(), "dx": xs.grad.cpu()}
    for name, idx in C.gelu_groups():
        for k in ("y", "dx"):
            _check(f"gelu(n={C.GELU_N}) {name}", k, out[k][idx], ref[k][idx], yd[k][idx], C.FWD_TOL)


@pytest.mark.parametrize("f", C.UPLIN_F)
@pytest.mark.parametrize("t", C.UPLIN_T)
def test_upsample_linear_backward_vs_fp64(t, f):
    from otpose_amd import hip
    from otpose_amd import train_ops as T
    d = C.uplin_inputs(t, f)
    ref, yd = E.upsample_linear(d["x"], f, d["dy"]), E.upsample_linear_yardstick(d["x"], f, d["dy"])
    xs = d["x"].cuda().requires_grad_()
    y = T.upsample_linear(xs, f)
    y.backward(d["dy"].cuda())
    name = f"upsample_linear(T={t}, f={f})"
    _check(name, "y", y, ref["y"], yd["y"], C.FWD_TOL)
    _check(name, "dx", xs.grad, ref["dx"], yd["dx"], C.FWD_TOL)
    # grad_out as a channel slice of a wider tensor, through the C interface
    (b, c), (ctot, coff) = C.UPLIN_BC, C.UPLIN_SLICE
    dy = d["wide"][:, coff: coff + c].contiguous()
    ref, yd = E.upsample_linear(d["x"], f, dy), E.upsample_linear_yardstick(d["x"], f, dy)
    wide, gx = d["wide"].cuda(), torch.full((b, c, t), NAN, device="cuda")
    hip.check(hip.lib().otp_upsample_linear_backward(hip.ptr(wide), hip.ptr(gx), b, c, t, f, ctot, coff, hip.stream_of(wide)),
              "otp_upsample_linear_backward")
    _check(name + f" slice {coff}..{coff + c - 1} of {ctot}", "dx", gx, ref["dx"], yd["dx"], C.FWD_TOL)


# ---- fuse rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("case", C.UPADD_CASES)
def test_upsample_add_backward_vs_fp64(case, relu):
    from otpose_amd import train as TR
    low_shape, f, branch = case
    d = C.upadd_inputs(low_shape, f, relu)
    ref, yd = E.upsample_add(d["low"], d["res"], f, relu, d["dy"]), E.upsample_add_yardstick(d["low"], d["res"], f, relu, d["dy"])
    low, res = d["low"].cuda().requires_grad_(), d["res"].cuda().requires_grad_()
    y = TR.UpsampleAddFunction.apply(low, res, f, relu)
    y.backward(d["dy"].cuda())
    name = f"upsample_add{low_shape} f={f} relu={int(relu)} {branch}"
    _check(name, "y", y, ref["y"], yd["y"], C.FWD_TOL)
    _check(name, "dres", res.grad, ref["dres"], yd["dres"], C.FWD_TOL)
    _check(name, "dlow", low.grad, ref["dlow"], yd["dlow"], C.FWD_TOL)
    if relu:
        zeros = d["zero"] & (ref["y"] == 0)
        assert int(zeros.sum()) >= C.UPADD_MIN_ZEROS
        assert float(y.detach().cpu()[zeros].abs().max()) == 0.0 and float(res.grad.cpu()[zeros].abs().max()) == 0.0
