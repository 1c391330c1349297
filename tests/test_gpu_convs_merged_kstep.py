"""The last k-step of a chunk in csrc/convs.hip (k-slots 16, 17 = tap 8 of the chunk's 16 input channels): its three half
products run as two MFMAs - lo * hi on lanes 0 .. 31 next to hi * lo on lanes 32 .. 63, then hi * hi - against a float64
``F.conv2d`` at 2e-5 of the output range.  Shapes: one chunk, partial cout blocks, NTW = 2 and 3, the BasicBlock conv2 form
with its S8 residual; weights that live on tap 8 only, so that nothing but the merged products carries the result; and the
bits of a launch when other kernels run before it."""
import pytest
import torch
import torch.nn.functional as F

from otpose_amd import ops

pytestmark = pytest.mark.gpu


def _operands(n, ci, co, h, w, seed, tap8_only=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, ci, h, w, generator=g) * 3
    wt = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (ci * 9)) ** 0.5
    if tap8_only:
        keep = torch.zeros(3, 3)
        keep[2, 2] = 1.0
        wt = wt * keep
    sc = torch.rand(co, generator=g) + 0.5
    sh = torch.randn(co, generator=g)
    res = torch.randn(n, co, h, w, generator=g)
    return x.cuda(), wt.cuda(), sc.cuda(), sh.cuda(), res.cuda()


def _ref(xs, shape, wt, sc, sh, res=None, relu=True):
    n, ci, h, w = shape
    xin = ops.s8_unpack(xs, n, ci, h, w).double()
    ref = F.conv2d(xin, wt.double(), None, 1, 1, 1) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    if res is not None:
        ref = ref + res.double()
    return torch.relu(ref) if relu else ref


def _check(y, ref):
    scale = float(ref.abs().max())
    err = float((y.double() - ref).abs().max()) / scale
    assert err <= 2e-5, err


# (N, Cin, Cout, H, W): Cout -> NTW (csrc/convs.hip s8_ntw): 16, 32, 64 -> 2; 48, 80 -> 3
CASES = [
    (2, 16, 16, 8, 4),        # one chunk, NTW = 2, one partial tile
    (3, 16, 48, 12, 8),       # one chunk, NTW = 3
    (2, 32, 80, 10, 6),       # Cout = 5 tiles: the second cout block holds 2 of 3 tiles (a lone one in the S8 store)
    (2, 80, 32, 10, 6),       # 5 chunks, NTW = 2
    (3, 80, 80, 12, 9),       # 5 chunks, partial cout block
    (4, 48, 48, 24, 18),      # NTW = 3, NPT = 2
    (5, 64, 64, 96, 72),      # NTW = 2, NPT = 4 (layer1 width)
    (5, 48, 48, 96, 72),      # NTW = 3, NPT = 4 (HRNet-W48 branch 0)
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
@pytest.mark.parametrize("tap8_only", [False, True], ids=["all_taps", "tap8_only"])
def test_merged_last_kstep_matches_float64(case, tap8_only):
    n, ci, co, h, w = case
    x, wt, sc, sh, _ = _operands(n, ci, co, h, w, sum(case) + int(tap8_only), tap8_only)
    xs = ops.s8_pack(x)
    y, ys = ops.conv3x3_s8(xs, (n, ci, h, w), wt, sc, sh, ops.ACT_RELU, None)
    _check(y, _ref(xs, (n, ci, h, w), wt, sc, sh))
    assert torch.equal(ys, ops.s8_pack(y))


@pytest.mark.parametrize("case", [c for c in CASES if c[1] == c[2]], ids=lambda c: "x".join(str(v) for v in c))
def test_conv2_form_with_s8_residual_matches_float64(case):
    n, ci, co, h, w = case
    x, wt, sc, sh, res = _operands(n, ci, co, h, w, 7 * sum(case))
    xs = ops.s8_pack(x)
    rs8 = ops.s8_pack(res)
    r_hl = ops.s8_unpack(rs8, n, co, h, w)                # the residual the kernel adds: hi + lo of its records
    y, ys = ops.conv3x3_s8(xs, (n, ci, h, w), wt, sc, sh, ops.ACT_RELU, res_s8=rs8)
    _check(y, _ref(xs, (n, ci, h, w), wt, sc, sh, r_hl))
    assert torch.equal(ys, ops.s8_pack(y))


def test_bits_stable_next_to_other_kernels():
    n, ci, co, h, w = 16, 48, 48, 96, 72
    x, wt, sc, sh, res = _operands(n, ci, co, h, w, 11)
    xs, rs8 = ops.s8_pack(x), ops.s8_pack(res)
    y0, ys0 = ops.conv3x3_s8(xs, (n, ci, h, w), wt, sc, sh, ops.ACT_RELU, res_s8=rs8)
    torch.cuda.synchronize()
    # other kernels in flight on the same stream and on a second one before the next launches
    other = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device="cuda")
    for k in range(3):
        with torch.cuda.stream(other):
            big = big @ big.t() * 1e-2
        ops.s8_pack(res)
        y1, ys1 = ops.conv3x3_s8(xs, (n, ci, h, w), wt, sc, sh, ops.ACT_RELU, res_s8=rs8)
        assert torch.equal(y1, y0) and torch.equal(ys1, ys0), k
    torch.cuda.synchronize()
