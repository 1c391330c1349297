"""Deformable PS-RoI pooling on the GPU (csrc/deform_pool.hip) against the numpy reference tests/deform_pool_ref.py.

Inputs come from ``guarded_case`` (no sample within 1e-3 of a line where the operator is discontinuous) and are rounded to
float32 first, so the fp32 kernel, the fp64 kernel and the reference all see the same numbers.

Bounds.  fp64: 1e-10 max-abs (about a hundred fp64 operations on O(1) values).  fp32: the reference is also evaluated with
every coordinate step in float32; e32 is that result's max-abs distance from the fp64 reference, and the kernel must be
within 4 * e32 + 1e-6 of the fp64 reference (4: a different but legitimate summation order and rounding of the weights).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_pool_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# (out_size, group_size, part_size, sample_per_part, num_classes)
CONFIGS = [(3, 3, 3, 2, 1), (4, 2, 2, 4, 2), (3, 1, 3, 1, 1), (2, 2, 1, 3, 4)]
LARGEST = (4, 2, 2, 4, 2)
CASES = [(c, nt) for c in CONFIGS for nt in (False, True)]
IDS = ["%d-%d-%d-%d-%d-%s" % (*c, "notrans" if nt else "trans") for c, nt in CASES]
DTYPES = [torch.float64, torch.float32]


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(cfg, no_trans):
    """One guarded case and everything the reference says about it; computed once, shared by every test, never modified."""
    data, rois, offset, grad_out, kw = R.guarded_case(11, *cfg, no_trans)
    data, offset, grad_out = _f32(data), _f32(offset), _f32(grad_out)
    rois = _f32(rois)
    off = None if no_trans else offset
    assert R.min_guard_distance(data.shape, rois, off, **kw) > R.GUARD              # still guarded after the rounding to float32
    ref = {"data": data, "rois": rois, "offset": offset, "grad_out": grad_out, "kw": kw}
    for name, ctype in (("64", np.float64), ("32", np.float32)):
        out, cnt = R.forward(data, rois, off, ctype=ctype, **kw)
        gin, goff = R.backward(grad_out, data, rois, off, cnt, ctype=ctype, **kw)
        ref["out" + name], ref["cnt" + name], ref["gin" + name], ref["goff" + name] = out, cnt, gin, goff
    assert np.array_equal(ref["cnt32"], ref["cnt64"])                                # what the guard is for
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _args(kw):
    return (kw["no_trans"], kw["spatial_scale"], kw["out_channels"], kw["group_size"], kw["out_size"], kw["part_size"],
            kw["sample_per_part"], kw["trans_std"])


def _bound(ref, what, dtype):
    if dtype == torch.float64:
        return 0.0, 1e-10
    e32 = float(np.abs(ref[what + "32"] - ref[what + "64"]).max())
    return e32, 4 * e32 + 1e-6


def _forward(ref, dtype):
    from otpose_amd import ops
    kw = ref["kw"]
    data, rois = _dev(ref["data"], dtype), _dev(ref["rois"], dtype)
    offset = data.new_empty(0) if kw["no_trans"] else _dev(ref["offset"], dtype)
    shape = ref["out64"].shape
    out, cnt = data.new_full(shape, 7.0), data.new_full(shape, 7.0)
    ops.deform_psroi_pooling_cuda_forward(data, rois, offset, out, cnt, *_args(kw))
    return data, rois, offset, out, cnt


def _pattern(shape, dtype, phase):
    n = int(np.prod(shape))
    return (0.5 * torch.sin(torch.arange(n, dtype=torch.float64) * 0.37 + phase)).reshape(shape).to("cuda", dtype)


def _backward(ref, dtype, fill):
    """The direct backward call into zero-filled (fill False) or pattern-filled buffers; returns them with their start values."""
    from otpose_amd import ops
    kw = ref["kw"]
    data, rois, offset, _, cnt = _forward(ref, dtype)
    gout = _dev(ref["grad_out"], dtype)
    oshape = ref["offset"].shape
    gin0 = _pattern(data.shape, dtype, 0.1) if fill else torch.zeros_like(data)
    goff0 = _pattern(oshape, dtype, 0.7) if fill else torch.zeros(oshape, device="cuda", dtype=dtype)
    gin, goff = gin0.clone(), goff0.clone()
    ops.deform_psroi_pooling_cuda_backward(gout, data, rois, offset, cnt, gin, goff, *_args(kw))
    return gin, goff, gin0, goff0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("cfg,no_trans", CASES, ids=IDS)
def test_forward(cfg, no_trans, dtype):
    ref = reference(cfg, no_trans)
    _, _, _, out, cnt = _forward(ref, dtype)
    assert out.dtype == dtype and cnt.dtype == dtype
    assert np.array_equal(cnt.cpu().numpy().astype(np.float64), ref["cnt64"])
    e32, bound = _bound(ref, "out", dtype)
    err = float(np.abs(out.double().cpu().numpy() - ref["out64"]).max())
    print("forward %s no_trans=%s %s: e32 %.3e  kernel error %.3e  bound %.3e" % (cfg, no_trans, dtype, e32, err, bound))
    assert err <= bound
    assert not out[2].any() and not cnt[2].any()                                     # the RoI outside the map


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("cfg,no_trans", CASES, ids=IDS)
def test_backward(cfg, no_trans, dtype):
    ref = reference(cfg, no_trans)
    for fill in (False, True):
        gin, goff, gin0, goff0 = _backward(ref, dtype, fill)
        e32, bound = _bound(ref, "gin", dtype)
        err = float(np.abs((gin.double() - gin0.double()).cpu().numpy() - ref["gin64"]).max()) if not fill else \
            float(np.abs(gin.double().cpu().numpy() - (gin0.double().cpu().numpy() + ref["gin64"])).max())
        print("grad_input %s no_trans=%s %s fill=%s: e32 %.3e  kernel error %.3e  bound %.3e"
              % (cfg, no_trans, dtype, fill, e32, err, bound))
        assert err <= bound
        if no_trans:
            assert torch.equal(goff, goff0)                                          # bit-unchanged
            continue
        e32, bound = _bound(ref, "goff", dtype)
        err = float(np.abs(goff.double().cpu().numpy() - (goff0.double().cpu().numpy() + ref["goff64"])).max())
        print("grad_offset %s %s fill=%s: e32 %.3e  kernel error %.3e  bound %.3e" % (cfg, dtype, fill, e32, err, bound))
        assert err <= bound
        assert torch.equal(goff[2], goff0[2])                                        # the RoI outside the map: no gradient


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_two_runs_are_bit_identical(dtype):
    ref = reference(LARGEST, False)
    a, b = _forward(ref, dtype), _forward(ref, dtype)
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    for fill in (False, True):
        a, b = _backward(ref, dtype, fill), _backward(ref, dtype, fill)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("no_trans", [False, True])
def test_autograd_matches_the_direct_call(no_trans):
    from otpose_amd import deform_roi_pooling, ops
    ref = reference(LARGEST, no_trans)
    kw = ref["kw"]
    dtype = torch.float32
    data, rois = _dev(ref["data"], dtype).requires_grad_(), _dev(ref["rois"], dtype).requires_grad_()
    offset = (data.new_empty(0) if no_trans else _dev(ref["offset"], dtype)).requires_grad_()
    out = deform_roi_pooling(data, rois, offset, kw["spatial_scale"], kw["out_size"], kw["out_channels"], no_trans,
                             kw["group_size"], kw["part_size"], kw["sample_per_part"], kw["trans_std"])
    _, _, _, want, cnt = _forward(ref, dtype)
    assert torch.equal(out, want)
    out.sum().backward()
    assert rois.grad is None
    gin, goff = torch.zeros_like(data), torch.zeros_like(offset)
    ops.deform_psroi_pooling_cuda_backward(torch.ones_like(want), data.detach(), rois.detach(), offset.detach(), cnt, gin, goff,
                                           *_args(kw))
    assert torch.equal(data.grad, gin) and gin.any()
    if not no_trans:
        assert torch.equal(offset.grad, goff) and goff.any()
    # part_size = None stands for out_size
    out2 = deform_roi_pooling(data.detach(), rois.detach(), data.new_empty(0), kw["spatial_scale"], kw["out_size"],
                              kw["out_channels"], True, kw["group_size"], None, kw["sample_per_part"], kw["trans_std"])
    want2 = torch.empty_like(want)
    ops.deform_psroi_pooling_cuda_forward(data.detach(), rois.detach(), None, want2, torch.empty_like(want), True,
                                          kw["spatial_scale"], kw["out_channels"], kw["group_size"], kw["out_size"],
                                          kw["out_size"], kw["sample_per_part"], kw["trans_std"])
    assert torch.equal(out2, want2)


def test_modulated_pack_with_its_zero_tails_is_half_the_plain_pooling():
    from otpose_amd import DeformRoIPoolingPack, ModulatedDeformRoIPoolingPack
    rng = np.random.RandomState(5)
    data = _f32(rng.uniform(-1, 1, size=(1, 18, 9, 7)))
    rois = _f32(np.array([[0, 1.2, 1.7, 4.3, 6.1], [0, 3.8, 5.2, 11.1, 13.3], [0, 0.5, 1.5, 3.5, 4.5]]))
    scale, trans_std = float(np.float32(0.87)), float(np.float32(0.1))
    kw = dict(no_trans=True, spatial_scale=scale, out_channels=18, group_size=1, out_size=3, part_size=3, sample_per_part=2,
              trans_std=trans_std)
    assert R.min_guard_distance(data.shape, rois, None, **kw) > R.GUARD
    want, _ = R.forward(data, rois, None, **kw)
    e32 = float(np.abs(R.forward(data, rois, None, ctype=np.float32, **kw)[0] - want).max())
    torch.manual_seed(0)
    x, r = _dev(data, torch.float32), _dev(rois, torch.float32)
    mod = ModulatedDeformRoIPoolingPack(scale, 3, 18, False, sample_per_part=2, trans_std=trans_std, deform_fc_channels=32).cuda()
    out = mod(x, r)
    assert out.shape == (3, 18, 3, 3)
    assert float(np.abs(out.detach().double().cpu().numpy() - 0.5 * want).max()) <= 4 * e32 + 1e-6      # sigmoid(0) = 0.5
    pack = DeformRoIPoolingPack(scale, 3, 18, False, sample_per_part=2, trans_std=trans_std, deform_fc_channels=32).cuda()
    out = pack(x, r)
    assert float(np.abs(out.detach().double().cpu().numpy() - want).max()) <= 4 * e32 + 1e-6
    out.sum().backward()                                                             # the offset branch receives a gradient
    assert pack.offset_fc[-1].weight.grad is not None and pack.offset_fc[-1].weight.grad.any()
    assert mod(x, r[:0]).shape == (0, 18, 3, 3) and pack(x, r[:0]).shape == (0, 18, 3, 3)


def test_rejected_calls_launch_nothing():
    from otpose_amd import ops
    ref = reference((3, 1, 3, 1, 1), False)
    kw = ref["kw"]
    data, rois, offset, out, cnt = _forward(ref, torch.float32)
    keep = out.clone()
    with pytest.raises(NotImplementedError):
        ops.deform_psroi_pooling_cuda_forward(data.cpu(), rois, offset, out, cnt, *_args(kw))
    with pytest.raises(RuntimeError, match="not implemented for torch.float16"):
        ops.deform_psroi_pooling_cuda_forward(data.half(), rois.half(), offset.half(), out.half(), cnt.half(), *_args(kw))
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        ops.deform_psroi_pooling_cuda_forward(data, rois.double(), offset, out, cnt, *_args(kw))
    wide = torch.cat([data, data[:, :1]], 1).contiguous()
    with pytest.raises(RuntimeError, match="wont match"):
        ops.deform_psroi_pooling_cuda_forward(wide, rois, offset, out, cnt, *_args(kw))
    with pytest.raises(RuntimeError, match="wont match"):
        ops.deform_psroi_pooling_cuda_backward(out, wide, rois, offset, cnt, torch.zeros_like(wide), torch.zeros_like(offset),
                                               *_args(kw))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.deform_psroi_pooling_cuda_forward(data.transpose(2, 3), rois, offset, out, cnt, *_args(kw))
    with pytest.raises(RuntimeError, match="wont match"):
        ops.deform_psroi_pooling_cuda_forward(data, rois[:3], offset, out, cnt, *_args(kw))
    torch.cuda.synchronize()
    assert torch.equal(out, keep)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("no_trans", [False, True])
def test_non_finite_grad_out_is_not_swallowed(no_trans, dtype):
    """One NaN and one inf in grad_out: the fixed-point plane cannot carry them, so every element of grad_input becomes NaN
    (the reference's atomicAdd would have carried them to the cells they touch); grad_offset receives them through its own sum."""
    from otpose_amd import ops
    ref = reference((3, 3, 3, 2, 1), no_trans)
    kw = ref["kw"]
    for bad in ((float("nan"),), (float("inf"),), (float("nan"), float("inf"))):
        data, rois, offset, _, cnt = _forward(ref, dtype)
        gout = _dev(ref["grad_out"], dtype)
        assert cnt[0, 0, 1, 1] > 0 and cnt[5, 1, 2, 0] > 0
        gout[0, 0, 1, 1] = bad[0]                                                    # RoI 0, class 0, part (1, 1)
        gout[5, 1, 2, 0] = bad[-1]                                                   # RoI 5, class 0, part (2, 0)
        gin = _pattern(data.shape, dtype, 0.1)
        goff0 = _pattern(ref["offset"].shape, dtype, 0.7)
        goff = goff0.clone()
        ops.deform_psroi_pooling_cuda_backward(gout, data, rois, offset, cnt, gin, goff, *_args(kw))
        assert torch.isnan(gin).all()
        if no_trans:
            assert torch.equal(goff, goff0)
            continue
        assert not torch.isfinite(goff[0, :, 1, 1]).any() and not torch.isfinite(goff[5, :, 2, 0]).any()
        if bad[0] != bad[0]:
            assert torch.isnan(goff[0, :, 1, 1]).all()
        untouched = torch.ones_like(goff, dtype=torch.bool)
        untouched[0, :, 1, 1] = False
        untouched[5, :, 2, 0] = False
        assert torch.isfinite(goff[untouched]).all()


def test_fractional_count_is_no_count():
    """out_count is the forward's output, whole numbers.  A caller's value in (0, 1) would make |grad_out / count| exceed the bound
    the fixed-point scale is built on; such an element is skipped like a count of 0."""
    from otpose_amd import ops
    ref = reference((3, 3, 3, 2, 1), False)
    kw = ref["kw"]
    data, rois, offset, _, cnt = _forward(ref, torch.float32)
    gout = _dev(ref["grad_out"], torch.float32)
    a = [torch.zeros_like(data), torch.zeros_like(offset)]
    b = [torch.zeros_like(data), torch.zeros_like(offset)]
    zero, frac = cnt.clone(), cnt.clone()
    zero[0, 0, 1, 1] = 0.0
    frac[0, 0, 1, 1] = 1e-3
    ops.deform_psroi_pooling_cuda_backward(gout, data, rois, offset, zero, *a, *_args(kw))
    ops.deform_psroi_pooling_cuda_backward(gout, data, rois, offset, frac, *b, *_args(kw))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].any()


@pytest.mark.parametrize("no_trans", [False, True])
def test_zero_rois(no_trans):
    """No RoI: the Function and the plain module return an empty (0, C, out_size, out_size) tensor, and zero gradients."""
    from otpose_amd import DeformRoIPooling
    data = torch.rand(2, 18, 9, 7, device="cuda", requires_grad=True)
    rois = torch.zeros(0, 5, device="cuda")
    offset = torch.zeros(0, 2, 3, 3, device="cuda", requires_grad=True)
    pool = DeformRoIPooling(0.9, 3, 2, no_trans, group_size=3, sample_per_part=2, trans_std=0.1)
    out = pool(data, rois, offset)
    assert out.shape == (0, 2, 3, 3) and out.dtype == data.dtype
    out.sum().backward()
    assert data.grad.shape == data.shape and not data.grad.any()
