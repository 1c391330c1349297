"""Case lists, inputs, host-rule restatements and bounds shared by tests/test_encoder_bwd_host.py (CPU) and
tests/test_gpu_encoder_bwd.py (the kernels).  No GPU import.

Every case carries the name of the branch it exists for; the ``*_branch`` functions below restate the host-side rules and the
in-kernel loops of csrc/transformer_bwd.hip, csrc/chanattn.hip and csrc/glue.hip from the case's numbers, and the host test
asserts that name and numbers agree, so an edit of a list cannot silently drop a branch.

Bounds are tests/reductions_cases.bound: 4 x the error of torch's fp32 CPU autograd on the same operands against float64, at
least 4 ulp of the reference's maximum, never above the cap - FWD_TOL for forwards and the input gradients of element-wise or
three-tap operators (GELU, max-pool, the up-samplings, the depthwise conv), GRAD_TOL for parameter gradients and for gradients
that pass through a reduction (LayerNorm's dx and dy * xhat, the softmax backward).  The attention gradients come from
bfloat16-piece products, which is not what torch's fp32 does: their bound is max(4 x yardstick, 2e-4 of the gradient's maximum),
capped at 2e-4 (the figure of tests/test_gpu_train_ops.py::test_chan_attn_backward)."""
import math

import torch

from tests import encoder_bwd_ref as E
from tests import reductions_cases as K

FWD_TOL, GRAD_TOL, ATTN_TOL = K.FWD_TOL, K.GRAD_TOL, 2e-4


def attn_bound(yard, ref):
    refmax = float(ref.abs().max())
    return min(max(4.0 * yard, ATTN_TOL * refmax), ATTN_TOL * max(1.0, refmax))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ---- depthwise conv --------------------------------------------------------------------------------------------------------
DWW_THREADS = 1024


def dwconv_branch(b, c, t, stride, offset=0):
    """dwconv3_bwd_w_kernel / the dX kernel choice: one vector rule (stride 1, T % 4 == 0, 16-byte aligned tensors - a contiguous
    view ``offset`` floats into an aligned buffer is aligned when offset % 4 == 0).  The float4 branch of dW walks B * T / 4
    groups: ``for (i = tid; i + 1024 < groups; i += 2048) two groups; if (i < groups) one more``."""
    if not (stride == 1 and t % 4 == 0 and offset % 4 == 0):
        return "scalar"
    groups = b * (t // 4)
    loop = tail = 0
    for tid in range(DWW_THREADS):
        i = tid
        ran = False
        while i + DWW_THREADS < groups:
            i += 2 * DWW_THREADS
            ran = True
        loop += ran
        tail += i < groups
    return f"float4 rows={t // 4} loop={loop} tail={tail}"


# (B, C, T, stride, storage offset of x and grad_y in floats, branch)
DWCONV_CASES = [
    (3, 5, 2740, 1, 0, "float4 rows=685 loop=1024 tail=7"),     # every thread runs the paired loop once, threads 0-6 the tail too
    (2, 5, 2400, 1, 0, "float4 rows=600 loop=176 tail=848"),    # threads 0-175 the loop, the others the tail only
    (1, 3, 4, 1, 0, "float4 rows=1 loop=0 tail=1"),             # one float4 per row: both neighbours outside the row
    (1, 3, 8, 1, 0, "float4 rows=2 loop=0 tail=2"),
    (2, 40, 101, 1, 0, "scalar"),
    (2, 7, 100, 2, 0, "scalar"),
    (2, 7, 101, 2, 0, "scalar"),
    (1, 2, 1, 2, 0, "scalar"),
    (1, 2, 2, 1, 0, "scalar"),
    (2, 136, 700, 1, 0, "float4 rows=175 loop=0 tail=350"),     # the channel count of the temporal encoders
    (2, 5, 400, 1, 1, "scalar"),                                # T % 4 == 0 but x and grad_y one float off 16-byte alignment
]


def dwconv_inputs(b, c, t, stride, offset=0, seed=0):
    """x and dy are contiguous views ``offset`` floats into their storage."""
    g = K.gen(7000 + seed)
    to = E.dwconv3_out_len(t, stride)

    def at_offset(*shape):
        n = math.prod(shape)
        buf = torch.zeros(offset + n)
        buf[offset:] = _randn(g, n)
        return buf[offset:].view(*shape)

    return {"x": at_offset(b, c, t), "dy": at_offset(b, c, to), "w": 0.5 * _randn(g, c, 1, 3), "prefill": _randn(g, c, 1, 3)}


# ---- channel LayerNorm -----------------------------------------------------------------------------------------------------
LN_SPLIT_MAX_C = 136


def ln_branch(c, t, direct=False):
    """``direct``: otp_ln_channel_backward (dx and dy * xhat out); else otp_ln_channel_backward_params as ``_ln_bwd`` of train_ops calls
    it whenever the library reports a workspace (C <= 136).  tiles = workgroups along T; last = tokens of the last one; the
    channel split over the waves as (channels per wave, channels of the last non-empty wave, empty waves)."""
    if c > LN_SPLIT_MAX_C:
        return f"generic tiles={-(-t // 256)} last={(t - 1) % 256 + 1}"
    wide = not direct and t % 4 == 0 and t >= 1024
    waves, tile = (8, 256) if wide else (4, 64)
    cw = -(-c // waves)
    full = c // cw
    used = full + (1 if c % cw else 0)
    kind = "wide" if wide else ("split-dyxh" if direct else "split-sums")
    return f"{kind} tiles={-(-t // tile)} last={(t - 1) % tile + 1} cw={cw} lastwave={c - (used - 1) * cw} empty={waves - used}"


# (B, C, T, mean offset m of x, branch)
LN_CASES = [
    (2, 1, 65, 0, "split-sums tiles=2 last=1 cw=1 lastwave=1 empty=3"),
    (2, 5, 65, 0, "split-sums tiles=2 last=1 cw=2 lastwave=1 empty=1"),
    (2, 17, 65, 0, "split-sums tiles=2 last=1 cw=5 lastwave=2 empty=0"),
    (2, 133, 65, 0, "split-sums tiles=2 last=1 cw=34 lastwave=31 empty=0"),
    (2, 136, 65, 0, "split-sums tiles=2 last=1 cw=34 lastwave=34 empty=0"),
    (2, 136, 63, 0, "split-sums tiles=1 last=63 cw=34 lastwave=34 empty=0"),
    (2, 136, 64, 0, "split-sums tiles=1 last=64 cw=34 lastwave=34 empty=0"),
    (3, 136, 300, 0, "split-sums tiles=5 last=44 cw=34 lastwave=34 empty=0"),
    (1, 136, 1020, 0, "split-sums tiles=16 last=60 cw=34 lastwave=34 empty=0"),     # T % 4 == 0, just under the wide rule
    (2, 136, 1023, 0, "split-sums tiles=16 last=63 cw=34 lastwave=34 empty=0"),     # T >= 1024 fails by one, T % 4 != 0
    (2, 136, 1024, 0, "wide tiles=4 last=256 cw=17 lastwave=17 empty=0"),           # the first T of the wide kernel, full tiles
    (2, 136, 1028, 0, "wide tiles=5 last=4 cw=17 lastwave=17 empty=0"),             # ragged 256-token tile: one live lane
    (2, 17, 1028, 0, "wide tiles=5 last=4 cw=3 lastwave=2 empty=2"),
    (1, 1, 1024, 0, "wide tiles=4 last=256 cw=1 lastwave=1 empty=7"),               # one channel: dx is exactly 0
    (2, 137, 70, 0, "generic tiles=1 last=70"),
    (2, 204, 300, 0, "generic tiles=2 last=44"),                                    # the 7-frame C, across a tile boundary
    (1, 204, 257, 0, "generic tiles=2 last=1"),
    # mean large against the spread: x = m + N(0, 1).  m = 32 is the largest of {4, 8, 16, 32} at which torch's fp32 autograd
    # still passes its caps against float64 - all four do.  The yardstick's error at m = 32 on the CPU: y 8.7e-6 (cap 1.9e-4),
    # dx 3.9e-6 (5.2e-4), dgamma 2.9e-4 (1.5e-2), dbeta 1.5e-5 (1.2e-2), dy * xhat 2.5e-5 (1.0e-3); dgamma's grows with m
    # (3.3e-5, 8.0e-5, 1.6e-4 at m = 4, 8, 16).  tests/test_encoder_bwd_host.py re-checks the choice.
    (2, 136, 1028, 32, "wide tiles=5 last=4 cw=17 lastwave=17 empty=0"),
]
LN_OFFSETS = (4, 8, 16, 32)
# otp_ln_channel_backward through ctypes: (B, C, T, branch)
LN_DIRECT_CASES = [
    (2, 17, 65, "split-dyxh tiles=2 last=1 cw=5 lastwave=2 empty=0"),
    (2, 136, 130, "split-dyxh tiles=3 last=2 cw=34 lastwave=34 empty=0"),
    (2, 136, 1024, "split-dyxh tiles=16 last=64 cw=34 lastwave=34 empty=0"),        # (this entry point has no wide kernel)
    (1, 204, 257, "generic tiles=2 last=1"),
]
LN_CAPS = {"y": FWD_TOL, "dx": GRAD_TOL, "dgamma": GRAD_TOL, "dbeta": GRAD_TOL, "dyxh": GRAD_TOL}


def ln_inputs(b, c, t, m=0, seed=0):
    g = K.gen(7100 + seed)
    x = (m + _randn(g, b, c, t)) if m else (2.0 * _randn(g, b, c, t) + 0.3)
    return {"x": x, "gamma": 1 + 0.1 * _randn(g, 1, c, 1), "beta": _randn(g, 1, c, 1), "dy": _randn(g, b, c, t)}


# ---- channel attention -----------------------------------------------------------------------------------------------------
ATT_TC = 64


def attn_splits(bh, t):
    """csrc/chanattn.hip: slices of T the score kernels work on (the library's otp_chan_attn_splits)."""
    ns = 1
    while bh * ns < 768 and t // (ns * 2) >= 2 * ATT_TC:
        ns *= 2
    return ns


def attn_branch(b, c, heads, t):
    hs = c // heads
    nb = (hs + 15) // 16
    return f"hs={hs} NB={nb} pad={nb * 16 - hs} tt={128 if nb > 6 else 256} splits={attn_splits(b * heads, t)}"


# (B, C, heads, T, factor on grad_out, branch); heads wider than 80 are the run-time LDS sizes, NB 7 the 128-step P.v tile
ATTN_CASES = [
    (2, 204, 2, 300, 1.0, "hs=102 NB=7 pad=10 tt=128 splits=2"),
    (2, 204, 2, 250, 1.0, "hs=102 NB=7 pad=10 tt=128 splits=1"),
    (1, 204, 2, 520, 1.0, "hs=102 NB=7 pad=10 tt=128 splits=4"),
    (2, 192, 2, 260, 1.0, "hs=96 NB=6 pad=0 tt=256 splits=2"),
    (1, 224, 2, 130, 1.0, "hs=112 NB=7 pad=0 tt=128 splits=1"),          # the widest head the kernels take
    (2, 32, 2, 70, 1.0, "hs=16 NB=1 pad=0 tt=256 splits=1"),
    (2, 136, 2, 520, 1.0, "hs=68 NB=5 pad=12 tt=256 splits=4"),
    (2, 204, 2, 300, 1e-8, "hs=102 NB=7 pad=10 tt=128 splits=2"),        # gradients of any magnitude keep their precision
]
WIDE_HEAD = 80


def attn_inputs(b, c, t, mag=1.0, seed=0):
    g = K.gen(7200 + seed)
    return {"q": 0.3 * _randn(g, b, c, t), "k": 0.3 * _randn(g, b, c, t), "v": _randn(g, b, c, t),
            "go": _randn(g, b, c, t) * mag}


SOFTMAX_BH = 3
SOFTMAX_CASES = [(hs, ns) for hs in (17, 64, 65, 102, 112) for ns in (1, 3)]


def softmax_inputs(hs, ns, seed=0):
    """slabs (BH, NS, HSP, HSP) and P (BH, HSP, HSP): P a real softmax over the first hs columns, both zero beyond hs."""
    g = K.gen(7300 + seed)
    hsp = (hs + 15) // 16 * 16
    slabs, p = torch.zeros(SOFTMAX_BH, ns, hsp, hsp), torch.zeros(SOFTMAX_BH, hsp, hsp)
    slabs[:, :, :hs, :hs] = _randn(g, SOFTMAX_BH, ns, hs, hs)
    p[:, :hs, :hs] = torch.softmax(2.0 * _randn(g, SOFTMAX_BH, hs, hs), dim=-1)
    return {"slabs": slabs, "p": p, "hsp": hsp}


# (batches, R, Cc): tiles of 32 x 32 - ragged both ways, across a tile edge, exactly one tile, a single row
TRANSPOSE_CASES = [(3, 70, 17), (2, 33, 65), (1, 32, 32), (2, 1, 102)]
TRANSPOSE_SCALES = [1.0, 0.5, 1.0 / math.sqrt(68)]


# ---- max-pool ----------------------------------------------------------------------------------------------------------------
POOL_ROWS = (3, 5)                                       # (B, C): 15 rows
POOL_T = [1, 2, 3, 77, 96, 511, 512, 513]                # the shortest rows, odd / even, the 256-thread tile edge of dx (T) and y (To)


def pool_inputs(t, seed=0):
    """Integers in [-2, 2] (ties in most windows); row 0 constant, row 1 strictly decreasing."""
    g = K.gen(7400 + seed)
    rows = POOL_ROWS[0] * POOL_ROWS[1]
    x = torch.randint(-2, 3, (rows, t), generator=g).float()
    x[0] = 1.0
    x[1] = torch.arange(t, 0, -1).float()
    return {"x": x, "dy": _randn(g, rows, (t + 2 - 3) // 2 + 1)}


# ---- GELU --------------------------------------------------------------------------------------------------------------------
GELU_N = 8192 * 256 + 257                                # one element per thread of the capped grid, then a ragged second pass
GELU_SMALL = [0.0, 1e-30, 1e-10, 1e-5, 1e-3, 0.1, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5, 8.0,
              8.5, 9.0]
GELU_LARGE = [10.0, 13.0, 14.0, 20.0, 38.0, 100.0, 1e3, 1e4]      # beyond the tail: gelu(x) = x or -0, gelu'(x) = 1 or 0


def gelu_inputs(seed=0):
    """N(0, 2) with the first 64 entries overwritten by +-GELU_SMALL, +-GELU_LARGE (pairs: +m at 2 i, -m at 2 i + 1)."""
    g = K.gen(7500 + seed)
    x, dy = 2.0 * _randn(g, GELU_N), _randn(g, GELU_N)
    mags = torch.tensor(GELU_SMALL + GELU_LARGE)
    assert mags.numel() == 32
    x[0:64:2], x[1:64:2] = mags, -mags
    return {"x": x, "dy": dy}


def gelu_groups():
    """(name, index) pairs: everything but the large specials as one tensor, then each large magnitude on its own - one bound for
    all would be 4 ulp of 1e4 and see nothing of the rest."""
    first_large = 2 * len(GELU_SMALL)
    bulk = torch.cat([torch.arange(first_large), torch.arange(64, GELU_N)])
    return [("bulk", bulk)] + [(f"|x|={m:g}", torch.tensor([first_large + 2 * i, first_large + 2 * i + 1]))
                               for i, m in enumerate(GELU_LARGE)]


# ---- linear up-sampling -------------------------------------------------------------------------------------------------------
UPLIN_BC = (2, 9)
UPLIN_F = [1, 2, 4]
UPLIN_T = [1, 2, 60, 255, 256, 257]                      # T = 1: no right neighbour anywhere; the 256-thread tile edge
UPLIN_SLICE = (16, 3)                                    # grad_out as channels 3 .. 11 of a 16-channel tensor (out_ctot, out_coff)


def uplin_inputs(t, f, seed=0):
    g = K.gen(7600 + seed)
    b, c = UPLIN_BC
    return {"x": _randn(g, b, c, t), "dy": _randn(g, b, c, t * f), "wide": _randn(g, b, UPLIN_SLICE[0], t * f)}


# ---- fuse rows: relu?(res + nearest_upsample_f(low)) --------------------------------------------------------------------------
def upadd_branch(low_shape, f):
    """otp_upsample_add: the float4 forward needs f in {2, 4, 8, 16} and a high-resolution width that is a multiple of 4."""
    return "vec" if f in (2, 4, 8, 16) and (low_shape[3] * f) % 4 == 0 else "scalar"


# (low shape, f, forward branch); every case runs with and without the ReLU
UPADD_CASES = [((2, 5, 3, 5), 2, "scalar"), ((2, 5, 3, 5), 4, "vec"), ((2, 5, 3, 5), 8, "vec"),
               ((1, 8, 4, 8), 2, "vec"), ((1, 8, 4, 8), 4, "vec"), ((1, 8, 4, 8), 8, "vec")]
UPADD_MIN_ZEROS = 10


def upadd_inputs(low_shape, f, relu, seed=0):
    """With the ReLU, res = -upsample(low) on a seeded tenth of the positions: the sum is exactly 0 there in any precision."""
    g = K.gen(7700 + seed)
    n, c, hl, wl = low_shape
    low = _randn(g, n, c, hl, wl)
    res, dy = _randn(g, n, c, hl * f, wl * f), _randn(g, n, c, hl * f, wl * f)
    zero = torch.rand(n, c, hl * f, wl * f, generator=g) < 0.1
    if relu:
        res = torch.where(zero, -E.nearest_up(low, f), res)
    return {"low": low, "res": res, "dy": dy, "zero": zero}
