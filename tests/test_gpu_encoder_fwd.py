"""The forward kernels of the temporal and flow encoders (csrc/dense.hip, densex.hip, mlp.hip, mlpx.hip, flowenc.hip, ln_channel and
dwconv_ln3 of csrc/transformer.hip) against float64 (tests/encoder_fwd_ref.py) at every tile edge, launch route and width:
tests/encoder_fwd_cases.py names the branch of each case and tests/test_encoder_fwd_host.py derives it again from the numbers.
The token tiles of the matrix kernels from T = 2 (nearly every lane clamped) across the 128 / 256 / 432-token workgroup edges with
one and three samples; launches of one to three dense problems with, without and with mixed residuals; the three mlpx forms and
the two of mlp.hip, each also in place on its residual; all four ln_channel kernels and the three wave splits and the generic
kernel of dwconv_ln3 by width, stride and padding; the flow encoder's hidden-unit split with idle waves; every in-kernel LayerNorm
on an input of mean 32 and spread of order 1 (x = 32 + N(0, 1), for the front ends and dwconv_ln3 through taps that sum to
about 1); the half-operand twins at the edge lengths.

Every output lives inside a buffer prefilled with a sentinel and 64 guard floats either side must come back bit-unchanged; every
launch runs twice and must repeat bit for bit; with three samples the middle one must equal its own single-sample run (its
neighbours across the sample edge are padding, not the other samples' tokens).

Bounds (tests/encoder_fwd_cases.py): exact-fp32 kernels 4 x the float32 CPU restatement's error, at least 4 ulp of the
reference's maximum, at most 3e-5 of max(1, max|ref|); split-product kernels 2e-5 of the output range; half-operand twins
4e-3 / 2e-3 / 2e-3 of the range against the split-product twins.  Every comparison prints ``ENCFWD|name|err|yardstick|bound``.

Measured on an MI355X (all 267 cases pass; per family: comparisons, largest kernel error, largest float32-yardstick error,
smallest bound, worst error / bound):
    dense_cc                    32   5.7e-06   6.7e-06   4.4e-06   0.34
    dense_x3                    66   5.3e-06   4.4e-06   8.1e-05   0.02
    dense_bf16p                 70   5.5e-05   4.4e-06   8.1e-05   0.28
    qkv_front_cc                48   2.6e-06   2.8e-06   3.5e-06   0.34
    qkv_front_cc m=32            6   2.8e-05   2.8e-05   7.7e-05   0.32
    qkv_front_x3                96   2.6e-06   2.8e-06   8.0e-05   0.02
    qkv_front_x3 m=32           12   3.0e-05   3.6e-05   1.0e-04   0.28
    mlp_fused                   24   7.4e-06   3.7e-06   6.5e-06   0.64
    ln_mlp_fused                24   9.2e-06   3.8e-06   4.7e-06   0.69
    ln_mlp_fused m=32            4   2.2e-05   2.6e-05   8.5e-05   0.21
    mlp_x3                      36   7.0e-06   4.5e-06   1.2e-04   0.03
    ln_mlp_x3                   36   6.3e-06   4.0e-06   1.2e-04   0.03
    ln_mlp_x3 m=32               8   3.4e-05   2.9e-05   8.3e-04   0.04
    ln_mlp_x3 m=32 out-res       8   3.4e-05   2.9e-05   1.7e-04   0.18
    ln_channel                 100   1.9e-06   1.1e-06   1.5e-08   0.65
    ln_channel m=32              8   3.0e-05   1.1e-05   2.7e-05   0.89
    dwconv_ln3                 486   4.7e-06   2.3e-06   1.5e-08   0.91
    dwconv_ln3 m=32             24   5.5e-05   5.3e-05   3.5e-05   0.72
    flow_front                  36   9.8e-07   1.1e-06   7.4e-07   0.46
    flow_front m=32              6   1.7e-05   1.9e-05   5.0e-05   0.26
    flow_back                   20   1.6e-06   1.5e-06   9.5e-07   0.33
    flow_back m=32               4   6.6e-06   5.4e-06   1.9e-05   0.30
    half-operand twins, fraction of the split-product twin's range: mlp <= 2.9e-04, dense <= 2.8e-04, qkv <= 3.3e-04
On unshifted inputs the split-product kernels stay at the float32 restatement's own error at the new edge lengths, a fiftieth of
their bound; on the shifted ones they follow the yardstick (the rounding of x = 32 + N(0, 1) itself).  The split-product
LN + MLP on the shifted input is held twice: its output to 2e-5 of a range the residual's + 32 inflates to about 42 - a float32
one-pass LayerNorm would sit about AT that bound - and ``out - res`` to 2e-5 of its own range plus half an ulp of the output, which
such a LayerNorm misses 4.6-fold (tests/test_encoder_fwd_host.py).  The worst exact-fp32 ratios are the generic (C > 204)
kernels of dwconv_ln3 and ln_channel, whose one thread per token sums the channels in index order.
"""
import math

import pytest
import torch

from tests import encoder_fwd_cases as C
from tests import reductions_cases as K

pytestmark = pytest.mark.gpu

D = torch.float64
GUARD = 64
SENTINEL = -7777.25


def _ops():
    from otpose_amd import ops
    return ops


def _guarded(shape):
    """(buffer, the output tensor inside it): sentinel everywhere, GUARD floats before and after the tensor."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[GUARD: GUARD + n].view(shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == 0
    return buf, out


def _guards_intact(buf, name):
    got = torch.cat([buf[:GUARD], buf[-GUARD:]]).view(torch.int32).cpu()
    want = torch.full((2 * GUARD,), SENTINEL, dtype=torch.float32).view(torch.int32)
    assert torch.equal(got, want), f"{name}: a store landed outside the output tensor"


def _twice(name, shapes, launch):
    """``launch(outs)`` into fresh guarded buffers, twice: guards unchanged, the second run bit-identical.  Returns the outputs."""
    runs = []
    for _ in range(2):
        bufs, outs = zip(*[_guarded(s) for s in shapes])
        launch(list(outs))
        torch.cuda.synchronize()
        for buf in bufs:
            _guards_intact(buf, name)
        runs.append(outs)
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), f"{name}: output {i} differs between two runs"
    return runs[0]


def _check(name, out, ref, yard_out, split):
    out = out.detach().cpu()
    assert bool(torch.isfinite(out).all()), f"{name}: inf or NaN"
    yard = K.max_err(yard_out, ref)
    assert yard <= C.FWD_TOL * max(1.0, float(ref.abs().max())), f"{name}: the fp32 yardstick itself is off by {yard}"
    err, bnd = K.max_err(out, ref), (C.x3_bound(ref) if split else K.bound(yard, ref, C.FWD_TOL))
    print(f"ENCFWD|{name}|{err:.3e}|{yard:.3e}|{bnd:.3e}")
    assert err <= bnd, f"{name}: max abs err {err} > {bnd} (fp32 yardstick {yard}, ref max {float(ref.abs().max())})"


def _in_place(name, res, launch, expect):
    """The same launch with the output aliased on the residual (a guarded copy of it): bit-equal to the out-of-place result."""
    buf, r = _guarded(res.shape)
    r.copy_(res)
    launch(r)
    torch.cuda.synchronize()
    _guards_intact(buf, name)
    assert torch.equal(r, expect), f"{name}: in place on the residual differs from out of place"


def _cuda(ts):
    return [t.cuda().contiguous() for t in ts]


# ops.ln_channel, ops.dwconv_ln3, ops.flow_front and ops.flow_back allocate their outputs themselves; to put the outputs between
# guards the same entry points are launched here with the arguments those wrappers state (ops.flow_front_args / flow_back_args,
# the argument order of ops.ln_channel / ops.dwconv_ln3), and each is first checked bit for bit against its wrapper.
def _ln_channel_into(x, g, be, eps, out):
    ops = _ops()
    b, c, t = x.shape
    ops.hip.check(ops.hip.lib().otp_ln_channel(ops.hip.ptr(x), ops.hip.ptr(g), ops.hip.ptr(be), ops.hip.ptr(out), None, b, c, t, eps,
                                                ops.hip.stream_of(x)), "otp_ln_channel")
    assert torch.equal(out, ops.ln_channel(x, g, be, eps))


def _dwconv_ln3_into(x, dws, gs, be, stride, eps, outs):
    ops = _ops()
    b, c, t = x.shape
    ptr = ops.hip.ptr
    ops.hip.check(ops.hip.lib().otp_dwconv_ln3(ptr(x), ptr(dws[0]), ptr(dws[1]), ptr(dws[2]), ptr(gs[0]), ptr(be[0]), ptr(gs[1]),
                                                ptr(be[1]), ptr(gs[2]), ptr(be[2]), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), b, c, t,
                                                stride, eps, ops.hip.stream_of(x)), "otp_dwconv_ln3")
    for got, want in zip(outs, ops.dwconv_ln3(x, dws, gs, be, stride, eps)):
        assert torch.equal(got, want)


def _flow_front_into(x, prm, eps, outs):
    ops = _ops()
    ops.hip.check(ops.hip.lib().otp_flow_front(*ops.flow_front_args(x, prm, *outs, eps), ops.hip.stream_of(x)), "otp_flow_front")
    for got, want in zip(outs, ops.flow_front(x, prm, eps)):
        assert torch.equal(got, want)


def _flow_back_into(x, att, prm, hidden, eps, out):
    ops = _ops()
    ops.hip.check(ops.hip.lib().otp_flow_back(*ops.flow_back_args(x, att, prm, out, hidden, eps), ops.hip.stream_of(x)), "otp_flow_back")
    assert torch.equal(out, ops.flow_back(x, att, prm, hidden, eps))


# ---- dense projections -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.DENSE_CASES, ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}-{''.join(map(str, k[3]))}")
def test_dense_vs_fp64(case):
    ops = _ops()
    entry, c, t, pattern, branch = case
    x3, grad = entry != "cc", entry == "bf16p"
    assert (ops.dense_x3_supported if x3 else ops.dense_cc_supported)(c, t) and C.dense_supported(entry, c, t)
    p = C.dense_params(c)
    sc = p["sc"].cuda()
    packs = [ops.pack_dense_cc(p["ws"][i].cuda(), sc if r else None, (p["bs"][i] * p["sc"]).cuda() if r else p["bs"][i].cuda(),
                               x3=x3, grad=grad) for i, r in enumerate(pattern)]
    for b in C.BATCHES:
        d = C.dense_inputs(c, b, t)
        xs = _cuda(d["xs"][:len(pattern)])
        ress = [d["res"][i].cuda() if r else None for i, r in enumerate(pattern)] if any(pattern) else None
        name = f"dense_{entry} C={c} B={b} T={t} res={''.join(map(str, pattern))} [{branch}]"
        outs = _twice(name, [(b, c, t)] * len(pattern), lambda o: ops.dense_cc(xs, packs, ress, o, x3=x3, grad=grad))
        ref, yd = C.dense_expected(c, b, t, pattern, D), C.dense_expected(c, b, t, pattern, torch.float32)
        for i in range(len(pattern)):
            _check(f"{name} #{i}", outs[i], ref[i], yd[i], x3)


# ---- q / k / v front end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.FRONT_CASES, ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}-m{k[3]}")
def test_qkv_front_vs_fp64(case):
    ops = _ops()
    entry, c, t, m, branch = case
    x3 = entry != "cc"
    p, dp = C.dw_params(c, bool(m)), C.dense_params(c)
    table = ops.pack_qkv_table(*_cuda(p["dws"]), *[v.cuda() for i in range(3) for v in (p["gs"][i], p["be"][i])])
    packs = [ops.pack_dense_cc(dp["ws"][i].cuda(), None, dp["bs"][i].cuda(), x3=x3) for i in range(3)]
    for b in C.BATCHES:
        x = C.shifted_input(c, b, t, m).cuda()
        name = f"qkv_front_{entry} C={c} B={b} T={t} m={m} [{branch}]"
        outs = _twice(name, [(b, c, t)] * 3, lambda o: ops.qkv_front(x, table, packs, 1e-5, o, x3=x3))
        ref, yd = C.front_expected(c, b, t, m, D), C.front_expected(c, b, t, m, torch.float32)
        for i, which in enumerate("qkv"):
            _check(f"{name} {which}", outs[i], ref[i], yd[i], x3)
        if b == 3:
            # the left neighbour of token 0 of sample 1 is padding, not sample 0's last token (and so on the right)
            alone = ops.qkv_front(x[1:2].contiguous(), table, packs, 1e-5, x3=x3)
            for i in range(3):
                assert torch.equal(outs[i][1:2], alone[i]), f"{name}: sample 1 depends on its neighbours in the batch"


# ---- MLP and LN + MLP --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.MLP_CASES, ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}-nt1{k[3]}-bal{k[4]}-m{k[5]}")
def test_mlp_vs_fp64(case, monkeypatch):
    ops = _ops()
    kernel, c, t, nt1, bal, m, branch = case
    for key, val in (("OTP_MLP_NT1", nt1), ("OTP_MLP_BALANCED", bal)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, val)
    split = kernel == "x3"
    assert (ops.mlp_x3_supported if split else ops.mlp_fused_supported)(c, 4 * c, t)
    p = {k: v.cuda() for k, v in C.mlp_params(c).items()}
    packed = (ops.pack_mlp_x3_weights if split else ops.pack_mlp_weights)(p["w1"].unsqueeze(2), p["b1"], p["w2"].unsqueeze(2))
    sc, sh = p["sc"], (C.mlp_params(c)["b2"] * C.mlp_params(c)["sc"]).cuda()
    f_mlp, f_ln = (ops.mlp_x3, ops.ln_mlp_x3) if split else (ops.mlp_fused, ops.ln_mlp_fused)
    for b in C.BATCHES:
        d = {k: v.cuda() for k, v in C.mlp_inputs(c, b, t, m).items()}
        ref, yd = C.mlp_expected(c, b, t, m, D), C.mlp_expected(c, b, t, m, torch.float32)
        name = f"{kernel} C={c} B={b} T={t} m={m} [{branch}]"
        if not m:
            (out,) = _twice(f"mlp_{name}", [(b, c, t)], lambda o: f_mlp(d["x"], packed, sc, sh, d["res"], out=o[0]))
            _check(f"mlp_{name}", out, ref["mlp"], yd["mlp"], split)
            _in_place(f"mlp_{name}", d["res"], lambda r: f_mlp(d["x"], packed, sc, sh, r, out=r), out)
        (out,) = _twice(f"ln_mlp_{name}", [(b, c, t)], lambda o: f_ln(d["res"], p["g"], p["be"], 1e-5, packed, sc, sh, out=o[0]))
        _check(f"ln_mlp_{name}", out, ref["ln_mlp"], yd["ln_mlp"], split)
        if split and m:
            # the MLP's own contribution, without the residual's + m in the range (encoder_fwd_cases.x3_branch_bound)
            res64 = C.mlp_inputs(c, b, t, m)["res"].to(D)
            err, bnd = K.max_err(out.cpu().to(D) - res64, ref["ln_mlp"] - res64), C.x3_branch_bound(ref["ln_mlp"], res64)
            print(f"ENCFWD|ln_mlp_{name} out-res|{err:.3e}|{K.max_err(yd['ln_mlp'], ref['ln_mlp']):.3e}|{bnd:.3e}")
            assert err <= bnd, f"ln_mlp_{name}: out - res is off by {err} > {bnd}"
        _in_place(f"ln_mlp_{name}", d["res"], lambda r: f_ln(r, p["g"], p["be"], 1e-5, packed, sc, sh, out=r), out)


# ---- channel LayerNorm -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.LN_CASES, ids=lambda k: f"{k[0]}-{k[1]}-m{k[2]}")
def test_ln_channel_vs_fp64(case):
    ops = _ops()
    c, t, m, branch = case
    for b in C.BATCHES:
        d = C.ln_inputs(b, c, t, m)
        x, g, be = d["x"].cuda(), d["gamma"].reshape(-1).cuda(), d["beta"].reshape(-1).cuda()
        name = f"ln_channel C={c} B={b} T={t} m={m} [{branch}]"
        (out,) = _twice(name, [(b, c, t)], lambda o: _ln_channel_into(x, g, be, 1e-5, o[0]))
        _check(name, out, C.ln_expected(c, b, t, m, D)[0], C.ln_expected(c, b, t, m, torch.float32)[0], False)


# ---- depthwise convs + LayerNorms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.DW_CASES, ids=lambda k: f"{k[0]}-s{k[1]}-{k[2]}-m{k[3]}")
def test_dwconv_ln3_vs_fp64(case):
    ops = _ops()
    c, stride, t, m, branch = case
    p = C.dw_params(c, bool(m))
    dws, gs, be = _cuda(p["dws"]), _cuda(p["gs"]), _cuda(p["be"])
    to = C.R.dwconv3_out_len(t, stride)
    for b in C.BATCHES:
        x = C.shifted_input(c, b, t, m, 8700).cuda()
        name = f"dwconv_ln3 C={c} B={b} m={m} [{branch}]"
        outs = _twice(name, [(b, c, to)] * 3, lambda o: _dwconv_ln3_into(x, dws, gs, be, stride, 1e-5, o))
        ref, yd = C.dwln_expected(c, b, t, stride, m, D), C.dwln_expected(c, b, t, stride, m, torch.float32)
        for i, which in enumerate("qkv"):
            _check(f"{name} {which}", outs[i], ref[i], yd[i], False)
        if b == 3:
            alone = ops.dwconv_ln3(x[1:2].contiguous(), dws, gs, be, stride, 1e-5)
            for i in range(3):
                assert torch.equal(outs[i][1:2], alone[i]), f"{name}: sample 1 depends on its neighbours in the batch"


# ---- flow encoder ------------------------------------------------------------------------------------------------------------
def _flow_params(hidden, t):
    """The hand-assembled parameter blocks the reference reads, checked against what ops.pack_flow_front / pack_flow_back build."""
    ops = _ops()
    blk = C.flow_block(hidden)
    assert ops.flow_block_supported(blk, C.FLOW_C, t)
    front, back = C.flow_front_block(blk), C.flow_back_block(blk)
    assert torch.equal(ops.pack_flow_front(blk, "cuda").cpu(), front) and torch.equal(ops.pack_flow_back(blk, "cuda").cpu(), back)
    return blk, front.cuda(), back.cuda()


@pytest.mark.parametrize("case", C.FLOW_FRONT_CASES, ids=lambda k: f"{k[0]}-m{k[1]}")
def test_flow_front_vs_fp64(case):
    ops = _ops()
    t, m, branch = case
    blk, front, _ = _flow_params(4 * C.FLOW_C, t)
    for b in C.BATCHES:
        x = C.flow_inputs(b, t, m)["x"].cuda()
        name = f"flow_front B={b} T={t} m={m} [{branch}]"
        outs = _twice(name, [(b, C.FLOW_C, t)] * 3, lambda o: _flow_front_into(x, front, blk.ln1.eps, o))
        ref, yd = C.flow_expected("front", 68, b, t, m, D), C.flow_expected("front", 68, b, t, m, torch.float32)
        for i, which in enumerate("qkv"):
            _check(f"{name} {which}", outs[i], ref[i], yd[i], False)
        if b == 3:
            alone = ops.flow_front(x[1:2].contiguous(), front, blk.ln1.eps)
            for i in range(3):
                assert torch.equal(outs[i][1:2], alone[i]), f"{name}: sample 1 depends on its neighbours in the batch"


@pytest.mark.parametrize("case", C.FLOW_BACK_CASES, ids=lambda k: f"H{k[0]}-{k[1]}-m{k[2]}")
def test_flow_back_vs_fp64(case):
    ops = _ops()
    hidden, t, m, branch = case
    blk, _, back = _flow_params(hidden, t)
    for b in C.BATCHES:
        d = {k: v.cuda() for k, v in C.flow_inputs(b, t, m).items()}
        name = f"flow_back B={b} T={t} m={m} [{branch}]"
        (out,) = _twice(name, [(b, C.FLOW_C, t)], lambda o: _flow_back_into(d["x"], d["att"], back, hidden, blk.ln2.eps, o[0]))
        _check(name, out, C.flow_expected("back", hidden, b, t, m, D)[0], C.flow_expected("back", hidden, b, t, m, torch.float32)[0],
               False)


# ---- half-operand twins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,t", C.H1_CASES)
def test_half_operand_twins_at_the_edge_lengths(c, t):
    """otp_ln_mlp_h1 / otp_dense_h1 / otp_qkv_front_h1 against their split-product twins on the same packed weights, by the
    criterion of tests/test_gpu_h16.py: 4e-3 / 2e-3 / 2e-3 of the range."""
    ops = _ops()
    b = C.H1_BATCH
    shape = (b, c, t)
    frac = lambda got, ref: float((got - ref).abs().max()) / float(ref.abs().max())          # noqa: E731
    p = {k: v.cuda() for k, v in C.mlp_params(c).items()}
    sh = (C.mlp_params(c)["b2"] * C.mlp_params(c)["sc"]).cuda()
    y = C.mlp_inputs(c, b, t, 0)["res"].cuda()
    w1, w2 = p["w1"].unsqueeze(2), p["w2"].unsqueeze(2)
    pk_x3, pk_h1 = ops.pack_mlp_x3_weights(w1, p["b1"], w2), ops.pack_mlp_x3_weights(w1, p["b1"], w2, half=True)
    ln = lambda pk, half: lambda o: ops.ln_mlp_x3(y, p["g"], p["be"], 1e-5, pk, p["sc"], sh, out=o[0], half=half)    # noqa: E731
    (ref,), (got,) = _twice(f"ln_mlp_x3 C={c} T={t}", [shape], ln(pk_x3, False)), _twice(f"ln_mlp_h1 C={c} T={t}", [shape], ln(pk_h1, True))
    e_mlp = frac(got, ref)
    dp = C.dense_params(c)
    d = C.dense_inputs(c, b, t)
    x, r = d["xs"][0].cuda(), d["res"][0].cuda()
    pk = ops.pack_dense_cc(dp["ws"][0].cuda(), dp["sc"].cuda(), (dp["bs"][0] * dp["sc"]).cuda(), x3=True)
    dense = lambda half: lambda o: ops.dense_cc([x], [pk], [r], o, x3=True, half=half)                                # noqa: E731
    (ref,), (got,) = _twice(f"dense_x3 C={c} T={t}", [shape], dense(False)), _twice(f"dense_h1 C={c} T={t}", [shape], dense(True))
    e_dense = frac(got, ref)
    q = C.dw_params(c)
    table = ops.pack_qkv_table(*_cuda(q["dws"]), *[v.cuda() for i in range(3) for v in (q["gs"][i], q["be"][i])])
    packs = [ops.pack_dense_cc(dp["ws"][i].cuda(), None, dp["bs"][i].cuda(), x3=True) for i in range(3)]
    xf = C.shifted_input(c, b, t, 0).cuda()
    front = lambda half: lambda o: ops.qkv_front(xf, table, packs, 1e-5, o, x3=True, half=half)                       # noqa: E731
    refs, gots = _twice(f"qkv_front_x3 C={c} T={t}", [shape] * 3, front(False)), _twice(f"qkv_front_h1 C={c} T={t}", [shape] * 3, front(True))
    e_qkv = max(frac(g_, r_) for g_, r_ in zip(gots, refs))
    for which, e in (("mlp", e_mlp), ("dense", e_dense), ("qkv", e_qkv)):
        print(f"ENCFWD|h1 {which} C={c} B={b} T={t} (fraction of the split-product twin's range)|{e:.3e}|0.000e+00|{C.H1_TOL[which]:.3e}")
    assert e_mlp <= C.H1_TOL["mlp"] and e_dense <= C.H1_TOL["dense"] and e_qkv <= C.H1_TOL["qkv"]
