"""Deformable PS-RoI pooling, the parts that need no GPU: the C ABI's symbols, the Python surface, the modules' parameters
against the reference's layout, and the numpy reference (tests/deform_pool_ref.py) checked by hand and against itself."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_pool_ref as R  # noqa: E402

# the configurations of tests/test_gpu_deform_pool.py: (out_size, group_size, part_size, sample_per_part, num_classes)
CONFIGS = [(3, 3, 3, 2, 1), (4, 2, 2, 4, 2), (3, 1, 3, 1, 1), (2, 2, 1, 3, 4)]


def test_library_exports_the_three_entry_points():
    from otpose_amd import hip
    cdll = ctypes.CDLL(hip.LIB_PATH)
    for name in ("otp_deform_psroi_pool_forward", "otp_deform_psroi_pool_backward", "otp_deform_psroi_pool_backward_workspace"):
        assert hasattr(cdll, name), name
        assert name in hip.SIGNATURES


def test_workspace_query_and_argument_codes():
    """Host-side argument checks of the C ABI: nothing is launched for a rejected call, so no GPU is needed."""
    from otpose_amd import hip
    cdll = ctypes.CDLL(hip.LIB_PATH)
    q = cdll.otp_deform_psroi_pool_backward_workspace
    q.restype, q.argtypes = hip.SIGNATURES["otp_deform_psroi_pool_backward_workspace"]
    # N, C, H, W, num_rois, offset_channels, no_trans, out_channels, G, pooled, part, spp, dtype
    assert q(2, 18, 9, 7, 6, 2, 0, 2, 3, 3, 3, 2, 0) == 8 * (2 * 18 * 9 * 7 + 1)
    assert q(2, 18, 9, 7, 6, 2, 0, 2, 3, 3, 3, 2, 1) == 0             # half: unsupported
    assert q(2, 17, 9, 7, 6, 2, 0, 2, 3, 3, 3, 2, 0) == 0             # C != out_channels * G^2
    f = cdll.otp_deform_psroi_pool_forward
    f.restype, f.argtypes = hip.SIGNATURES["otp_deform_psroi_pool_forward"]
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(C=18, offset_channels=2, out_channels=2, dtype=0, data=p, num_rois=6, N=2, H=9, W=7):
        return f(data, p, p, p, p, N, C, H, W, num_rois, offset_channels, 0, 1.0, out_channels, 3, 3, 3, 2, 0.1, dtype, None)
    assert fwd(data=None) == -1                                        # OTP_ERR_BAD_ARG
    assert fwd(num_rois=0) == -1
    assert fwd(C=17) == -1
    assert fwd(offset_channels=3) == -1
    assert fwd(C=27, out_channels=3, offset_channels=4) == -1          # 3 channels do not split into 2 classes
    assert fwd(dtype=1) == -2 and fwd(dtype=2) == -2                   # OTP_ERR_UNSUPPORTED
    assert fwd(N=1 << 12, H=1 << 8, W=1 << 8) == -2                   # N C H W >= 2^31
    assert fwd(num_rois=1 << 27) == -2                                 # n * out_channels * pooled^2 >= 2^31


def test_python_surface():
    import otpose_amd
    from otpose_amd import deform_pool, ops
    for name in ("DeformRoIPoolingFunction", "deform_roi_pooling", "DeformRoIPooling", "DeformRoIPoolingPack",
                 "ModulatedDeformRoIPoolingPack"):
        assert hasattr(deform_pool, name) and getattr(otpose_amd, name) is getattr(deform_pool, name)
    assert issubclass(deform_pool.DeformRoIPoolingFunction, torch.autograd.Function)
    for cls in (deform_pool.DeformRoIPooling, deform_pool.DeformRoIPoolingPack, deform_pool.ModulatedDeformRoIPoolingPack):
        assert issubclass(cls, torch.nn.Module)
    assert callable(ops.deform_psroi_pooling_cuda_forward) and callable(ops.deform_psroi_pooling_cuda_backward)


def test_cpu_tensors_are_refused():
    from otpose_amd import deform_roi_pooling, ops
    data, rois = torch.zeros(1, 4, 5, 5), torch.zeros(1, 5)
    out = torch.zeros(1, 4, 2, 2)
    with pytest.raises(NotImplementedError):
        ops.deform_psroi_pooling_cuda_forward(data, rois, data.new_empty(0), out, out.clone(), True, 1.0, 4, 1, 2, 2, 2, 0.0)
    with pytest.raises(NotImplementedError):
        ops.deform_psroi_pooling_cuda_backward(out, data, rois, data.new_empty(0), out, torch.zeros_like(data),
                                               data.new_empty(0), True, 1.0, 4, 1, 2, 2, 2, 0.0)
    with pytest.raises(NotImplementedError):
        deform_roi_pooling(data, rois, data.new_empty(0), 1.0, 2, 4, True)
    with pytest.raises(AssertionError):
        deform_roi_pooling(data, rois, data.new_empty(0), 1.0, 2, 4, True, 1, None, 4, 1.5)    # trans_std outside [0, 1]


def test_module_parameters_match_the_reference_layout():
    """state_dict keys and shapes read off the reference's modules/deform_pool.py (out_size 3, out_channels 4, 16 fc channels)."""
    from otpose_amd import DeformRoIPooling, DeformRoIPoolingPack, ModulatedDeformRoIPoolingPack
    offset_fc = {"offset_fc.0.weight": (16, 36), "offset_fc.0.bias": (16,), "offset_fc.2.weight": (16, 16),
                 "offset_fc.2.bias": (16,), "offset_fc.4.weight": (18, 16), "offset_fc.4.bias": (18,)}
    mask_fc = {"mask_fc.0.weight": (16, 36), "mask_fc.0.bias": (16,), "mask_fc.2.weight": (9, 16), "mask_fc.2.bias": (9,)}

    def shapes(m):
        return {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes(DeformRoIPooling(0.25, 3, 4, False)) == {}
    pack = DeformRoIPoolingPack(0.25, 3, 4, False, deform_fc_channels=16)
    assert shapes(pack) == offset_fc
    assert list(pack.state_dict()) == list(offset_fc)
    mod = ModulatedDeformRoIPoolingPack(0.25, 3, 4, False, deform_fc_channels=16)
    assert shapes(mod) == {**offset_fc, **mask_fc}
    assert list(mod.state_dict()) == list(offset_fc) + list(mask_fc)
    for m in (pack, mod):
        assert not m.offset_fc[-1].weight.any() and not m.offset_fc[-1].bias.any()
        assert m.offset_fc[0].weight.any()
        assert (m.part_size, m.group_size, m.sample_per_part, m.trans_std) == (3, 1, 4, .0)
    assert not mod.mask_fc[-2].weight.any() and not mod.mask_fc[-2].bias.any()
    assert isinstance(mod.mask_fc[-1], torch.nn.Sigmoid) and isinstance(mod.offset_fc[1], torch.nn.ReLU)
    assert shapes(DeformRoIPoolingPack(0.25, 3, 4, True)) == {} and shapes(ModulatedDeformRoIPoolingPack(0.25, 3, 4, True)) == {}
    assert DeformRoIPooling(1.0, 5, 4, True, part_size=2).part_size == 2


# ---- the numpy reference, by hand ------------------------------------------------------------------------------------------------
def test_reference_one_roi_one_bin_by_hand():
    """plane[y, x] = 3 y + x; RoI (0, 0)-(1, 1): edges -0.5 and 1.5, one 2 x 2 bin, samples at w, h in {-0.5, 0.5}.  -0.5 is not
    below the border: it is kept and clamped to 0.  Values 0, 0.5, 1.5, 2 -> mean 1, count 4."""
    data = np.arange(9.0).reshape(1, 1, 3, 3)
    rois = np.array([[0, 0, 0, 1, 1.0]])
    out, cnt = R.forward(data, rois, None, True, 1.0, 1, 1, 1, 1, 2, 0.0)
    assert cnt.item() == 4 and out.item() == 1.0
    # offsets (0.25, 0.5) at trans_std 0.5 move the bin by (0.125, 0.25) of the RoI's 2 x 2: w in {-0.25 -> 0, 0.75}, h in {0, 1};
    # values 0, 0.75, 3, 3.75 -> mean 1.875
    offset = np.array([0.25, 0.5]).reshape(1, 2, 1, 1)
    out, cnt = R.forward(data, rois, offset, False, 1.0, 1, 1, 1, 1, 2, 0.5)
    assert cnt.item() == 4 and out.item() == 1.875
    # and its backward: d out / d data spreads 1/4 per sample over its neighbours; d out / d offset_x = mean of df/dw * 0.5 * 2
    gin, goff = R.backward(np.ones((1, 1, 1, 1)), data, rois, offset, cnt, False, 1.0, 1, 1, 1, 1, 2, 0.5)
    want = np.zeros((3, 3))
    want[0, 0] += 0.25 + 0.25 * 0.25          # (0, 0) and the left neighbour of (0.75, 0)
    want[0, 1] += 0.25 * 0.75
    want[1, 0] += 0.25 + 0.25 * 0.25
    want[1, 1] += 0.25 * 0.75
    assert np.array_equal(gin[0, 0], want)
    # at an integer coordinate floor = ceil: the neighbours coincide and their difference is 0.  So the samples clamped to w = 0
    # give 0 and those at w = 0.75 give plane[., 1] - plane[., 0] = 1: (0 + 1 + 0 + 1) / 4 * trans_std * roi_width = 0.5;
    # h = 0 and h = 1 are integers: no gradient in y
    assert goff[0, 0, 0, 0] == 0.5 and goff[0, 1, 0, 0] == 0.0


def test_reference_rounds_halves_away_from_zero():
    """x1 = x2 = 2.5 -> 3 (numpy's round would give 2): the one sample sits at w = 2.5 of a plane holding its column index."""
    assert [R.round_half_away(v) for v in (0.5, 1.5, 2.5, -0.5, -2.5, 2.4999, 3.0)] == [1, 2, 3, -1, -3, 2, 3]
    data = np.tile(np.arange(8.0), (1, 1, 1, 1))
    out, cnt = R.forward(data, np.array([[0, 2.5, 0, 2.5, 0.0]]), None, True, 1.0, 1, 1, 1, 1, 1, 0.0)
    assert cnt.item() == 1 and out.item() == 2.5


def test_reference_minimum_roi_size_and_outside():
    data = np.arange(63.0).reshape(1, 1, 9, 7)
    # x2 < x1: width max((1 + 1 - 4), 0.1) = 0.1 -> the 2 samples of a row are 0.05 apart, starting at 3.5
    out, cnt = R.forward(data, np.array([[0, 4, 2, 1, 2.0]]), None, True, 1.0, 1, 1, 1, 1, 2, 0.0)
    assert cnt.item() == 4 and abs(out.item() - (7 * 1.75 + 3.525)) < 1e-12
    out, cnt = R.forward(data, np.array([[0, 20, 30, 24, 33.0]]), None, True, 1.0, 1, 1, 1, 1, 2, 0.0)
    assert cnt.item() == 0 and out.item() == 0.0


# ---- the case generator and the reference against itself -----------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("no_trans", [False, True])
def test_guarded_case_is_found_and_holds_every_roi_kind(cfg, no_trans):
    for seed in (0, 1):
        data, rois, offset, grad_out, kw = R.guarded_case(seed, *cfg, no_trans)       # asserts: accepted within 200 draws
        args = (rois, None if no_trans else offset)
        assert R.min_guard_distance(data.shape, *args, **kw) > R.GUARD
        assert kw["spatial_scale"] == float(np.float32(kw["spatial_scale"])) and kw["trans_std"] == float(np.float32(0.1))
        assert data.shape == (2, 2 * cfg[4] * cfg[1] ** 2, 9, 7)
        assert np.abs(offset).max() <= 1 and np.abs(data).max() <= 1
        _, cnt = R.forward(data, *args, **kw)
        full = cfg[3] ** 2
        assert (cnt[0] == full).all() and (cnt[5] == full).all()                      # inside; batch index 1
        assert (cnt[1] < full).any() and (cnt[1] > 0).any()                           # over the right and bottom borders
        assert (cnt[2] == 0).all()                                                    # outside
        assert rois[3, 3] < rois[3, 1] and rois[5, 0] == 1
        assert (np.modf(rois[4, 1:])[0] == 0.5).all()


def _loss(data, rois, offset, grad_out, kw):
    return float((R.forward(data, rois, offset, **kw)[0] * grad_out).sum())


@pytest.mark.parametrize("cfg", CONFIGS)
def test_reference_backward_agrees_with_finite_differences(cfg):
    """Central differences (step 1e-6, fp64) of sum(forward * grad_out) along random directions: the forward is linear in data
    and, away from the guarded lines, bilinear in each offset, so the difference quotient is exact up to its rounding,
    about 1e-16 / 1e-6 of the terms' size.  Error relative to sum |g_i v_i| <= 1e-6."""
    data, rois, offset, grad_out, kw = R.guarded_case(2, *cfg, False)
    _, cnt = R.forward(data, rois, offset, **kw)
    gin, goff = R.backward(grad_out, data, rois, offset, cnt, **kw)
    assert np.abs(gin).max() > 0 and np.abs(goff).max() > 0
    assert not goff[2].any()                                                          # the RoI outside the map
    rng = np.random.RandomState(3)
    eps = 1e-6
    for _ in range(2):
        v = rng.uniform(-1, 1, size=data.shape)
        fd = (_loss(data + eps * v, rois, offset, grad_out, kw) - _loss(data - eps * v, rois, offset, grad_out, kw)) / (2 * eps)
        assert abs(fd - (gin * v).sum()) <= 1e-6 * np.abs(gin * v).sum()
        v = rng.uniform(-1, 1, size=offset.shape)
        fd = (_loss(data, rois, offset + eps * v, grad_out, kw) - _loss(data, rois, offset - eps * v, grad_out, kw)) / (2 * eps)
        assert abs(fd - (goff * v).sum()) <= 1e-6 * np.abs(goff * v).sum()


def test_reference_backward_per_element_on_the_smallest_case():
    """Every offset and a sample of data elements one by one (configuration (3, 1, 3, 1, 1)): relative to the largest gradient."""
    data, rois, offset, grad_out, kw = R.guarded_case(4, 3, 1, 3, 1, 1, False)
    _, cnt = R.forward(data, rois, offset, **kw)
    gin, goff = R.backward(grad_out, data, rois, offset, cnt, **kw)
    eps = 1e-6
    fd = np.zeros_like(offset)
    for i in np.ndindex(*offset.shape):
        d = np.zeros_like(offset)
        d[i] = eps
        fd[i] = (_loss(data, rois, offset + d, grad_out, kw) - _loss(data, rois, offset - d, grad_out, kw)) / (2 * eps)
    assert np.abs(fd - goff).max() <= 1e-6 * np.abs(goff).max()
    # and element by element, relative to the difference quotient itself.  The quotient carries the rounding of the two sums it
    # subtracts: each is a sum of size S = sum |out * grad_out| known to 2^-53 S at best, so 2 * 2^-53 S / (2 eps) * 2 = 2^-52 S / eps
    # is the floor below which an element's quotient says nothing (it matters for the few gradients near 1e-4)
    out, _ = R.forward(data, rois, offset, **kw)
    floor = 2.0 ** -52 * np.abs(out * grad_out).sum() / eps
    assert (np.abs(fd - goff) <= 1e-6 * np.abs(fd) + floor).all()
    assert (np.abs(fd) > 1e3 * floor).sum() > offset.size // 2          # most elements are checked well above the floor
    hit = np.argwhere(gin != 0)
    assert len(hit) > 20
    for i in map(tuple, hit[::max(1, len(hit) // 40)]):
        d = np.zeros_like(data)
        d[i] = eps
        f = (_loss(data + d, rois, offset, grad_out, kw) - _loss(data - d, rois, offset, grad_out, kw)) / (2 * eps)
        assert abs(f - gin[i]) <= 1e-6 * np.abs(gin).max()
    # without offsets the data gradient is the same function of the (now unmoved) samples, and no offset gradient exists
    kw_nt = dict(kw, no_trans=True)
    _, cnt = R.forward(data, rois, None, **kw_nt)
    gin_nt, none = R.backward(grad_out, data, rois, None, cnt, **kw_nt)
    gin_0, _ = R.backward(grad_out, data, rois, np.zeros_like(offset), cnt, **kw)
    assert none is None and np.array_equal(gin_nt, gin_0)
