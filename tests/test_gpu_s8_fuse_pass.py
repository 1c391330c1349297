"""The streaming passes of the HRNet fuse rows (csrc/convs.hip: otp_s8_upsample_add / otp_s8_upsample_add_ex -> s8_fuse_pass_kernel,
otp_s8_pack -> s8_pack_kernel) against a float32 CPU restatement with the same order of additions and a host-side hi / lo split:
every output word must be equal, no tolerance.  Shapes are the smallest that reach every branch of the kernels: one, two and
three terms, an odd number of row pairs and a single one, partial last blocks, rows that are no multiple of the wave, C a
multiple of 8 but not 16, an odd N, and maps on both sides of the launcher's 32-bit index bound (beyond it the one-pixel kernel
runs)."""
import ctypes
import itertools

import pytest
import torch

from otpose_amd import hip, ops

pytestmark = pytest.mark.gpu

PAD = 8                                                              # channels in front of the slice in the wider NCHW tensors


def _h16(x):
    return x.to(torch.float16).to(torch.float32)


def _split(x):
    hi = _h16(x)
    return hi, _h16(x - hi)


def _s8_image(x):
    """host-side S8 image of an fp32 (n, c, h, w) tensor: [n][c/8][part][p][e] 16-bit pieces, as the int32 words ops.s8_empty holds"""
    n, c, h, w = x.shape
    hi, lo = _split(x)
    rec = torch.stack([hi, lo], 0).view(2, n, c // 8, 8, h * w).permute(1, 2, 0, 4, 3).contiguous()
    return rec.to(torch.float16).view(torch.int16).reshape(-1).view(torch.int32)


def _c4_image(x):
    n, c, h, w = x.shape
    return x.reshape(n, c // 4, 4, h * w).permute(0, 1, 3, 2).contiguous().reshape(-1)


def _inputs(n, c, hh, wh, factors, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(n, c, hh, wh, generator=g) * 3
    lows = [torch.randn(n, c, hh // f, wh // f, generator=g) * 2 for f in factors]
    raw[0, 1, 0, :2] = 0.0                                           # exact zeros: 0 + 0 (+ 0 ...) on the first row pair
    raw[-1, c - 1, hh - 1, wh - 1] = 0.0                             # and in the last pixel of the last plane
    for t in lows:
        t[0, 1, 0, 0] = 0.0
        t[-1, c - 1, -1, -1] = 0.0
    return raw, lows


def _reference(res, lows, factors, relu):
    o = res.clone()
    for t, f in zip(lows, factors):                                  # same order of additions as the kernel: ((res + l0) + l1) + l2
        o = o + t.repeat_interleave(f, 2).repeat_interleave(f, 3)
    return torch.relu(o) if relu else o


def _launch(lows_gpu, factors, res_gpu, res_layout, out_full, s8, c4, n, c, hh, wh, relu, res_ctot, res_coff):
    lp = (ctypes.c_void_p * len(lows_gpu))(*[hip.ptr(t) for t in lows_gpu])
    fp = (ctypes.c_int * len(factors))(*factors)
    hip.check(hip.lib().otp_s8_upsample_add_ex(lp, fp, len(factors), hip.ptr(res_gpu), res_layout, hip.ptr(out_full), hip.ptr(s8),
                                               hip.ptr(c4), n, c, hh, wh, int(relu), res_ctot, res_coff, c + PAD, PAD,
                                               hip.stream_of(s8)), "otp_s8_upsample_add_ex")


# (N, C, Hh, Wh, factors)
CASES = [
    (2, 16, 8, 16, (2,)),
    (2, 16, 8, 16, (2, 4)),
    (2, 16, 8, 16, (2, 4, 8)),
    (1, 48, 12, 36, (2, 4)),             # rows are no multiple of the wave, a partial last block
    (3, 24, 4, 8, (2,)),                 # C a multiple of 8 but not 16, odd N
    (1, 16, 10, 8, (2,)),                # five row pairs
    (1, 16, 2, 8, (2,)),                 # one row pair: the first is the last
    (1, 8, 2, 32768, (2,)),              # the longest rows the two-row kernel takes at this height ((Hh Wh / 2) Wh < 2^32) ...
    (1, 8, 2, 65536, (2,)),              # ... and the first beyond: the one-pixel kernel
]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "x".join(str(v) for v in c[:4]) + "_f" + "".join(str(f) for f in c[4]))
def case(request):
    n, c, hh, wh, factors = request.param
    raw, lows = _inputs(n, c, hh, wh, factors, seed=hh * wh + len(factors))
    hi, lo = _split(raw)
    res_s8_value = hi + lo                                           # what the kernel widens an S8 residual to
    full = torch.full((n, c + PAD, hh, wh), -5.0)
    full[:, PAD:] = raw
    return {
        "dims": (n, c, hh, wh), "factors": factors,
        "lows": lows, "lows_gpu": [t.cuda() for t in lows],
        "res": {0: raw, 1: res_s8_value},
        "res_gpu": {0: full.cuda(), 1: _s8_image(raw).cuda()},
        "ref": {(lay, relu): _reference(r, lows, factors, relu) for lay, r in ((0, raw), (1, res_s8_value)) for relu in (0, 1)},
    }


@pytest.mark.parametrize("res_layout", [0, 1], ids=["res_nchw_slice", "res_s8"])
def test_fuse_pass_equals_cpu_restatement(case, res_layout):
    n, c, hh, wh = case["dims"]
    for relu, with_nchw, with_c4 in itertools.product((0, 1), (False, True), (False, True)):
        ref = case["ref"][(res_layout, relu)]
        out_full = torch.full((n, c + PAD, hh, wh), 7.0, device="cuda") if with_nchw else None
        s8 = ops.s8_empty(n, c, hh, wh, "cuda").fill_(-1)
        c4 = ops.c4_empty(n, c, hh, wh, "cuda").fill_(-1.0) if with_c4 else None
        _launch(case["lows_gpu"], case["factors"], case["res_gpu"][res_layout], res_layout, out_full, s8, c4, n, c, hh, wh, relu,
                c + PAD, PAD)
        what = (relu, with_nchw, with_c4)
        assert torch.equal(s8.cpu(), _s8_image(ref)), what
        assert torch.equal(ops.s8_unpack(s8, n, c, hh, wh).cpu(), sum(_split(ref))), what
        if with_c4:
            assert torch.equal(c4.cpu(), _c4_image(ref)), what
        if with_nchw:
            got = out_full.cpu()
            assert torch.equal(got[:, PAD:], ref), what
            assert bool((got[:, :PAD] == 7.0).all()), what


def test_fuse_pass_record_words_equal_upsample_add_multi_then_pack(case):
    """the raw record words against the two-launch form on the GPU: otp_upsample_add_multi, then otp_s8_pack (S8 + C4)"""
    n, c, hh, wh = case["dims"]
    factors, lows_gpu, full = case["factors"], case["lows_gpu"], case["res_gpu"][0]
    lp = (ctypes.c_void_p * len(lows_gpu))(*[hip.ptr(t) for t in lows_gpu])
    fp = (ctypes.c_int * len(factors))(*factors)
    want = torch.empty(n, c, hh, wh, device="cuda")
    hip.check(hip.lib().otp_upsample_add_multi(lp, fp, len(factors), hip.ptr(full), hip.ptr(want), n, c, hh, wh, 1, c + PAD, PAD, c, 0,
                                               hip.stream_of(full)), "otp_upsample_add_multi")
    want_c4 = ops.c4_empty(n, c, hh, wh, "cuda")
    want_s8 = ops.s8_pack(want, out_c4=want_c4)
    s8, c4 = ops.s8_empty(n, c, hh, wh, "cuda"), ops.c4_empty(n, c, hh, wh, "cuda")
    _launch(lows_gpu, factors, full, 0, None, s8, c4, n, c, hh, wh, 1, c + PAD, PAD)
    assert torch.equal(s8, want_s8) and torch.equal(c4, want_c4)


@pytest.mark.range_overflow_expected
@pytest.mark.parametrize("res_layout", [0, 1], ids=["res_nchw_slice", "res_s8"])
def test_fuse_pass_raises_the_range_word(res_layout):
    """a sum at the half limit (65504) sets the S8 passes' code, before the ReLU and whatever the residual layout"""
    n, c, hh, wh, factors = 2, 16, 8, 16, (2, 4)
    raw, lows = _inputs(n, c, hh, wh, factors, seed=5)
    lows_gpu = [t.cuda() for t in lows]
    full = torch.zeros(n, c + PAD, hh, wh)
    full[:, PAD:] = raw
    s8 = ops.s8_empty(n, c, hh, wh, "cuda")

    def run(low0):
        res = full.cuda() if res_layout == 0 else _s8_image(raw).cuda()
        _launch([low0] + lows_gpu[1:], factors, res, res_layout, None, s8, None, n, c, hh, wh, 1, c + PAD, PAD)
        torch.cuda.synchronize()
        return hip.lib().otp_range_flag_read(1)

    hip.lib().otp_range_flag_read(1)
    assert run(lows_gpu[0]) == 0
    big = lows_gpu[0].clone()
    big[1, 9, 3, 7] = 65504.0 + 40.0                                 # (the residual under it is a few units: the sum stays >= 65504)
    assert run(big) == 6
    neg = lows_gpu[0].clone()
    neg[0, 0, 0, 0] = -7.0e4                                         # a negative one: tested before the ReLU hides it
    assert run(neg) == 6


@pytest.mark.parametrize("shape", [(2, 16, 5, 12), (1, 48, 12, 36)], ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("with_c4", [False, True], ids=["s8", "s8_c4"])
def test_s8_pack_of_a_channel_slice_equals_the_host_split(shape, with_c4):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(c * h + w)
    full = torch.randn(n, c + PAD + 8, h, w, generator=g) * 3
    full[0, PAD, 0, 0] = 0.0
    full[-1, PAD + c - 1, h - 1, w - 1] = -0.0
    x = full[:, PAD:PAD + c].contiguous()
    s8 = ops.s8_empty(n, c, h, w, "cuda").fill_(-1)
    c4 = ops.c4_empty(n, c, h, w, "cuda").fill_(-1.0) if with_c4 else None
    ops.s8_pack(ops.View(full.cuda(), PAD, c), out=s8, out_c4=c4)
    assert torch.equal(s8.cpu(), _s8_image(x))
    assert torch.equal(ops.s8_unpack(s8, n, c, h, w).cpu(), sum(_split(x)))
    if with_c4:
        assert torch.equal(c4.cpu(), _c4_image(x))
