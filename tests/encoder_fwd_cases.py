"""Case lists, inputs, host-rule restatements and bounds shared by tests/test_encoder_fwd_host.py (CPU) and
tests/test_gpu_encoder_fwd.py (the kernels): the forward kernels of the temporal and flow encoders - csrc/dense.hip, densex.hip,
mlp.hip, mlpx.hip, flowenc.hip and ln_channel / dwconv_ln3 of csrc/transformer.hip.  No GPU import, no hip.lib().

Every case carries the name of the branch it exists for, as literal text; the ``*_branch`` functions below restate the host-side
launch rules and the in-kernel index arithmetic from the case's numbers, and the host test asserts that text and numbers agree and
that every branch the functions can produce is named by a case - so an edit of a list cannot silently drop a branch.  Where a
family is a product (widths x lengths) the two factors carry their halves of the text and the cases are their product.

Bounds.  Exact-fp32 kernels (dense.hip, mlp.hip, flowenc.hip, ln_channel, dwconv_ln3): tests/reductions_cases.bound with
FWD_TOL - 4 x the error of the float32 CPU restatement (tests/encoder_fwd_ref.py on the same operands) against float64, at
least 4 ulp of the reference's maximum, never above 3e-5 of max(1, max|ref|).  Split-product kernels (densex.hip, mlpx.hip, the
bfloat16-piece dense included): 2e-5 of the output range, the figure of tests/test_gpu_ops.py::test_mlp_x3_matches_fp64.  The
half-operand twins: 4e-3 / 2e-3 / 2e-3 of the range against their split-product twins
(tests/test_gpu_h16.py::test_encoder_kernels_with_half_operands_stay_within_half_rounding_of_the_split_products).

Shifted inputs.  Every kernel with a LayerNorm inside also runs on x = m + N(0, 1); m is the largest of LN_OFFSETS at which the
float32 CPU yardstick still passes its cap against float64, as tests/encoder_bwd_cases.py chose it.  All four offsets pass for
every family, so m = 32 throughout, and tests/test_encoder_fwd_host.py re-checks the choice.  The yardstick's largest error at
m = 32 against its cap of 3e-5 max(1, max|ref|), per family: q/k/v front end 3.6e-5 (cap 1.9e-4), LN + MLP 2.9e-5 (1.3e-3),
ln_channel 1.1e-5 at C = 260, 1.0e-5 at C = 5, 8.0e-6 at C = 204, 7.4e-6 at C = 136 (2.0e-4), dwconv_ln3 5.3e-5 (2.0e-4),
flow_front 1.9e-5 (1.2e-4), flow_back 5.4e-6 (1.1e-3).  The front ends and dwconv_ln3 normalise the depthwise conv's output, not x,
so their shifted cases take taps that sum to about 1 (:func:`dw_params`); the host test asserts for every shifted case that what
each LayerNorm sees has a mean of more than ten times its spread (30 to 39 here), and that a float32 one-pass
``E[x^2] - mean^2`` LayerNorm put into the restatement misses the case's bound by more than a factor of two (4.6 to 19)."""
import functools

import numpy as np
import torch

from tests import encoder_fwd_ref as R
from tests import reductions_cases as K
from tests.encoder_bwd_cases import LN_OFFSETS, ln_inputs  # noqa: F401  (the LayerNorm operands are the backward suite's)

FWD_TOL = K.FWD_TOL
X3_TOL = 2e-5
H1_TOL = {"mlp": 4e-3, "dense": 2e-3, "qkv": 2e-3}
BATCHES = (1, 3)                      # b = blockIdx.x / tiles_per_b with nothing to divide and with two sample edges
M = 32                                # the mean offset of the shifted cases


def x3_bound(ref):
    return X3_TOL * max(1.0, float(ref.abs().max()))


def x3_branch_bound(ref, res):
    """The split-product LN + MLP on a shifted input, second check: the residual's + m inflates the output range and with it
    :func:`x3_bound`, but not the kernel's error - the products make up ``out - res`` and the residual is added last in float32.
    So ``out - res`` is held to 2e-5 of ITS range plus the one rounding of that addition, half an ulp of the output's maximum."""
    half_ulp = 0.5 * float(np.spacing(np.float32(float(ref.abs().max()))))
    return X3_TOL * max(1.0, float((ref - res).abs().max())) + half_ulp


def layer_norm_one_pass(x, gamma, beta, eps=1e-5):
    """The rewrite the shifted cases exist to catch: variance as E[x^2] - mean^2 in the operands' own precision."""
    mu = x.mean(1, keepdim=True)
    var = (x * x).mean(1, keepdim=True) - mu * mu
    return (x - mu) / torch.sqrt(var.clamp_min(0) + eps) * gamma.reshape(1, -1, 1) + beta.reshape(1, -1, 1)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ---- token tiles of the matrix kernels -----------------------------------------------------------------------------------------
def token_tile_branch(t, wg_tokens, waves, nt):
    """A workgroup of ``waves`` waves owns ``wg_tokens`` tokens; lane (kq = lane / 16, n = lane % 16) of a wave holds token
    ``tile * wg_tokens + wave * 16 nt + nt n`` (and the next one when nt = 2): ``valid = tok < T``, lanes that are not valid are
    clamped onto the last token (pair) and store nothing.  Counted in the last workgroup of a sample, the only ragged one."""
    tiles = -(-t // wg_tokens)
    clamped = idle = 0
    for wave in range(waves):
        live = 0
        for lane in range(64):
            tok = (tiles - 1) * wg_tokens + wave * 16 * nt + nt * (lane & 15)
            live += tok < t
            clamped += tok >= t
        idle += live == 0
    return f"tiles={tiles} last={t - (tiles - 1) * wg_tokens} clamped={clamped} idle_waves={idle}"


# ---- dense.hip / densex.hip: otp_dense_cc, otp_dense_x3, otp_dense_x3_bf16p -------------------------------------------------------
DENSE_WIDTHS = {"cc": (136,), "x3": (136, 204), "bf16p": (136, 204)}         # otp_dense_cc_supported / otp_dense_x3_supported


def dense_supported(entry, c, t):
    return c in DENSE_WIDTHS[entry] and t > 0 and t % 2 == 0


def dense_branch(t):
    """dense_cc_kernel / densex_cc_kernel: 128 tokens per workgroup, 32 per wave, a token pair per lane; grid (B * tiles, nprob)."""
    return token_tile_branch(t, 128, 4, 2)


# (T, branch)
DENSE_T = [
    (2, "tiles=1 last=2 clamped=252 idle_waves=3"),
    (30, "tiles=1 last=30 clamped=196 idle_waves=3"),
    (32, "tiles=1 last=32 clamped=192 idle_waves=3"),
    (34, "tiles=1 last=34 clamped=188 idle_waves=2"),
    (126, "tiles=1 last=126 clamped=4 idle_waves=0"),
    (128, "tiles=1 last=128 clamped=0 idle_waves=0"),
    (130, "tiles=2 last=2 clamped=252 idle_waves=3"),
    (258, "tiles=3 last=2 clamped=252 idle_waves=3"),
]
# residual pattern per problem of one launch (1: with residual and scale, like proj; 0: bias only, like query / key / value).
# A launch may mix them: ``res`` is a per-problem pointer, the exact-fp32 kernel tests it (``if (res)``) and the split-product
# one reads a zero-length buffer descriptor in its place, so (1, 0, 1) is a legal call and is listed.
DENSE_PATTERNS = [(0,), (1,), (0, 0), (1, 1), (0, 0, 0), (1, 1, 1), (1, 0, 1)]
DENSE_ENTRIES = [(e, c) for e in ("cc", "x3", "bf16p") for c in DENSE_WIDTHS[e]]
# (entry, C, T, pattern, branch): every entry at every T; the patterns rotate so that each entry sees all seven
DENSE_CASES = [(e, c, t, DENSE_PATTERNS[(ei + ti) % len(DENSE_PATTERNS)], br)
               for ei, (e, c) in enumerate(DENSE_ENTRIES) for ti, (t, br) in enumerate(DENSE_T)]


@functools.lru_cache(maxsize=None)
def dense_params(c):
    g = K.gen(8000 + c)
    return {"ws": [_randn(g, c, c) / c ** 0.5 for _ in range(3)], "bs": [_randn(g, c) for _ in range(3)], "sc": _randn(g, c)}


@functools.lru_cache(maxsize=None)
def dense_inputs(c, b, t):
    g = K.gen(8100 + 7 * c + 3 * t + b)
    return {"xs": [_randn(g, b, c, t) for _ in range(3)], "res": [_randn(g, b, c, t) for _ in range(3)]}


def dense_expected(c, b, t, pattern, dtype):
    """The launch's outputs in ``dtype`` (float64: the reference; float32: the yardstick)."""
    p, d = dense_params(c), dense_inputs(c, b, t)
    cast = lambda v: v.to(dtype)                                                       # noqa: E731
    return [R.pointwise(cast(d["xs"][i]), cast(p["ws"][i]), cast(p["bs"][i]), cast(p["sc"]) if r else None,
                        cast(d["res"][i]) if r else None) for i, r in enumerate(pattern)]


# ---- dense.hip / densex.hip: otp_qkv_front, otp_qkv_front_x3 ---------------------------------------------------------------------
FRONT_ENTRIES = [("cc", 136), ("x3", 136), ("x3", 204)]


def front_branch(t):
    """qkv_front_kernel / qkvx_front_kernel: the token tiles of :func:`dense_branch`; a lane that is not valid takes
    ``tokc = T - 2``; the depthwise conv's neighbours are masked by ``l_ok = tokc >= 1`` and ``r_ok = tokc + 2 < T``.  Counted over
    all workgroups of one sample: lanes whose left / right neighbour is padding (each token pair is held by four lanes)."""
    tiles = -(-t // 128)
    l_false = r_false = 0
    for tile in range(tiles):
        for wave in range(4):
            for lane in range(64):
                tok = tile * 128 + wave * 32 + 2 * (lane & 15)
                tokc = tok if tok < t else t - 2
                l_false += not tokc >= 1
                r_false += not tokc + 2 < t
    return f"{token_tile_branch(t, 128, 4, 2)} l_false={l_false} r_false={r_false}"


# (T, mean offset m, branch); at m = 32 the float32 yardstick is off by 3.6e-5 (cap 1.9e-4)
FRONT_T = [
    (2, 0, "tiles=1 last=2 clamped=252 idle_waves=3 l_false=256 r_false=256"),
    (30, 0, "tiles=1 last=30 clamped=196 idle_waves=3 l_false=4 r_false=200"),
    (32, 0, "tiles=1 last=32 clamped=192 idle_waves=3 l_false=4 r_false=196"),
    (34, 0, "tiles=1 last=34 clamped=188 idle_waves=2 l_false=4 r_false=192"),
    (126, 0, "tiles=1 last=126 clamped=4 idle_waves=0 l_false=4 r_false=8"),
    (128, 0, "tiles=1 last=128 clamped=0 idle_waves=0 l_false=4 r_false=4"),
    (130, 0, "tiles=2 last=2 clamped=252 idle_waves=3 l_false=4 r_false=256"),
    (258, 0, "tiles=3 last=2 clamped=252 idle_waves=3 l_false=4 r_false=256"),
    (130, 32, "tiles=2 last=2 clamped=252 idle_waves=3 l_false=4 r_false=256"),
]
FRONT_CASES = [(e, c, t, m, br) for e, c in FRONT_ENTRIES for t, m, br in FRONT_T]


@functools.lru_cache(maxsize=None)
def dw_params(c, shifted=False):
    """Depthwise weights and LayerNorm gamma / beta of the query / key / value paths.  ``shifted`` (the cases on x = m + N(0, 1)):
    taps 1/3 + 0.01 N(0, 1), whose sum is 1 to within 2 % in every channel, so that the conv output - what the LayerNorm inside these
    kernels normalises - keeps a mean of about m over a spread of order 1; zero-mean taps would turn m into spread."""
    g = K.gen(8200 + c + (1000 if shifted else 0))
    taps = (lambda: 1.0 / 3.0 + 0.01 * _randn(g, c, 1, 3)) if shifted else (lambda: 0.6 * _randn(g, c, 1, 3))
    return {"dws": [taps() for _ in range(3)], "gs": [1.0 + 0.3 * _randn(g, c) for _ in range(3)],
            "be": [0.2 * _randn(g, c) for _ in range(3)]}


@functools.lru_cache(maxsize=None)
def shifted_input(c, b, t, m, seed=8300):
    return m + _randn(K.gen(seed + 7 * c + 3 * t + b), b, c, t)


def front_expected(c, b, t, m, dtype):
    p, d, x = dw_params(c, bool(m)), dense_params(c), shifted_input(c, b, t, m)
    cast = lambda vs: [v.to(dtype) for v in vs]                                        # noqa: E731
    return R.qkv_front(x.to(dtype), cast(p["dws"]), cast(p["gs"]), cast(p["be"]), cast(d["ws"]), cast(d["bs"]))


# ---- mlp.hip / mlpx.hip: otp_mlp_fused, otp_ln_mlp_fused, otp_mlp_x3, otp_ln_mlp_x3 ---------------------------------------------
MLP_WIDTHS = {"fused": (136,), "x3": (136, 204)}                                       # (hidden = 4 C)
BALANCED_TOKENS = 27 * 16


def balanced_table():
    """mlp_fused_balanced_kernel / mlpx_balanced_kernel: the 27 sixteen-token tiles of a workgroup over its eight waves - pass 1
    two tiles each; pass 2 waves 0-2 two more, waves 4, 5, 6 -> 22, 23, 24, wave 3 -> 25, wave 7 -> 26 (one tile, one token per lane)."""
    own = {w: [2 * w, 2 * w + 1] for w in range(8)}
    for w in range(8):
        if w < 3:
            own[w] += [16 + 2 * w, 17 + 2 * w]
        else:
            own[w] += [25 if w == 3 else (26 if w == 7 else 18 + w)]
    assert sorted(tile for tiles in own.values() for tile in tiles) == list(range(27))
    return " ".join(f"w{w}:" + "+".join(map(str, own[w][2:])) for w in range(8))


def mlp_branch(kernel, c, b, t, nt1=None, bal=None):
    """mlp_launch (csrc/mlp.hip) and mlpx_launch (csrc/mlpx.hip) with the environment's OTP_MLP_NT1 / OTP_MLP_BALANCED."""
    bal_off, bal_force = bal is not None and bal[0] == "0", bal is not None and bal[0] == "2"
    balanced = not bal_off and t % BALANCED_TOKENS == 0 and (bal_force or b * (t // BALANCED_TOKENS) >= 192)
    if kernel == "fused":
        if balanced:
            return f"mlp balanced per_b={t // BALANCED_TOKENS} pass2={balanced_table()}"
        return "mlp nt2x4 " + token_tile_branch(t, 128, 4, 2)
    if c == 204:
        return "mlpx204 nt1x8 " + token_tile_branch(t, 128, 8, 1)
    if not (nt1 is not None and nt1[0] == "0") and not bal_force:
        return "mlpx nt1x8 " + token_tile_branch(t, 128, 8, 1)
    if balanced:
        return f"mlpx balanced per_b={t // BALANCED_TOKENS} pass2={balanced_table()}"
    return "mlpx nt2x8 " + token_tile_branch(t, 256, 8, 2)


# (kernel, C, T, OTP_MLP_NT1, OTP_MLP_BALANCED, mean offset m of the LayerNorm's input, branch); with m the case runs the
# LN + MLP entry alone, else the plain and the LN entries and both with the output aliased on the residual; at m = 32 the
# float32 yardstick is off by 2.6e-5 (C = 136) and 2.9e-5 (C = 204), cap 1.3e-3
MLP_CASES = [
    ("fused", 136, 2, None, None, 0, "mlp nt2x4 tiles=1 last=2 clamped=252 idle_waves=3"),
    ("fused", 136, 14, None, None, 0, "mlp nt2x4 tiles=1 last=14 clamped=228 idle_waves=3"),
    ("fused", 136, 16, None, None, 0, "mlp nt2x4 tiles=1 last=16 clamped=224 idle_waves=3"),
    ("fused", 136, 18, None, None, 0, "mlp nt2x4 tiles=1 last=18 clamped=220 idle_waves=3"),
    ("fused", 136, 30, None, None, 0, "mlp nt2x4 tiles=1 last=30 clamped=196 idle_waves=3"),     # the 32-token wave edge of mlp.hip
    ("fused", 136, 32, None, None, 0, "mlp nt2x4 tiles=1 last=32 clamped=192 idle_waves=3"),
    ("fused", 136, 34, None, None, 0, "mlp nt2x4 tiles=1 last=34 clamped=188 idle_waves=2"),
    ("fused", 136, 126, None, None, 0, "mlp nt2x4 tiles=1 last=126 clamped=4 idle_waves=0"),
    ("fused", 136, 128, None, None, 0, "mlp nt2x4 tiles=1 last=128 clamped=0 idle_waves=0"),
    ("fused", 136, 130, None, None, 0, "mlp nt2x4 tiles=2 last=2 clamped=252 idle_waves=3"),
    ("x3", 136, 2, None, None, 0, "mlpx nt1x8 tiles=1 last=2 clamped=504 idle_waves=7"),
    ("x3", 136, 14, None, None, 0, "mlpx nt1x8 tiles=1 last=14 clamped=456 idle_waves=7"),
    ("x3", 136, 16, None, None, 0, "mlpx nt1x8 tiles=1 last=16 clamped=448 idle_waves=7"),
    ("x3", 136, 18, None, None, 0, "mlpx nt1x8 tiles=1 last=18 clamped=440 idle_waves=6"),
    ("x3", 136, 126, None, None, 0, "mlpx nt1x8 tiles=1 last=126 clamped=8 idle_waves=0"),
    ("x3", 136, 128, None, None, 0, "mlpx nt1x8 tiles=1 last=128 clamped=0 idle_waves=0"),
    ("x3", 136, 130, None, None, 0, "mlpx nt1x8 tiles=2 last=2 clamped=504 idle_waves=7"),
    ("x3", 136, 30, "0", None, 0, "mlpx nt2x8 tiles=1 last=30 clamped=452 idle_waves=7"),
    ("x3", 136, 32, "0", None, 0, "mlpx nt2x8 tiles=1 last=32 clamped=448 idle_waves=7"),
    ("x3", 136, 34, "0", None, 0, "mlpx nt2x8 tiles=1 last=34 clamped=444 idle_waves=6"),
    ("x3", 136, 254, "0", None, 0, "mlpx nt2x8 tiles=1 last=254 clamped=4 idle_waves=0"),
    ("x3", 136, 256, "0", None, 0, "mlpx nt2x8 tiles=1 last=256 clamped=0 idle_waves=0"),
    ("x3", 136, 258, "0", None, 0, "mlpx nt2x8 tiles=2 last=2 clamped=508 idle_waves=7"),
    ("fused", 136, 432, None, "2", 0, "mlp balanced per_b=1 pass2=w0:16+17 w1:18+19 w2:20+21 w3:25 w4:22 w5:23 w6:24 w7:26"),
    ("fused", 136, 864, None, "2", 0, "mlp balanced per_b=2 pass2=w0:16+17 w1:18+19 w2:20+21 w3:25 w4:22 w5:23 w6:24 w7:26"),
    ("x3", 136, 432, None, "2", 0, "mlpx balanced per_b=1 pass2=w0:16+17 w1:18+19 w2:20+21 w3:25 w4:22 w5:23 w6:24 w7:26"),
    ("x3", 136, 864, None, "2", 0, "mlpx balanced per_b=2 pass2=w0:16+17 w1:18+19 w2:20+21 w3:25 w4:22 w5:23 w6:24 w7:26"),
    ("x3", 204, 2, None, None, 0, "mlpx204 nt1x8 tiles=1 last=2 clamped=504 idle_waves=7"),
    ("x3", 204, 126, None, None, 0, "mlpx204 nt1x8 tiles=1 last=126 clamped=8 idle_waves=0"),
    ("x3", 204, 130, None, None, 0, "mlpx204 nt1x8 tiles=2 last=2 clamped=504 idle_waves=7"),
    ("fused", 136, 130, None, None, 32, "mlp nt2x4 tiles=2 last=2 clamped=252 idle_waves=3"),
    ("x3", 136, 130, None, None, 32, "mlpx nt1x8 tiles=2 last=2 clamped=504 idle_waves=7"),
    ("x3", 136, 258, "0", None, 32, "mlpx nt2x8 tiles=2 last=2 clamped=508 idle_waves=7"),
    ("x3", 136, 432, None, "2", 32, "mlpx balanced per_b=1 pass2=w0:16+17 w1:18+19 w2:20+21 w3:25 w4:22 w5:23 w6:24 w7:26"),
    ("fused", 136, 432, None, "2", 32, "mlp balanced per_b=1 pass2=w0:16+17 w1:18+19 w2:20+21 w3:25 w4:22 w5:23 w6:24 w7:26"),
    ("x3", 204, 130, None, None, 32, "mlpx204 nt1x8 tiles=2 last=2 clamped=504 idle_waves=7"),
]


@functools.lru_cache(maxsize=None)
def mlp_params(c):
    g = K.gen(8400 + c)
    hid = 4 * c
    return {"w1": _randn(g, hid, c) / c ** 0.5, "b1": 0.5 * _randn(g, hid), "w2": _randn(g, c, hid) / hid ** 0.5,
            "b2": _randn(g, c), "sc": _randn(g, c), "g": 1.0 + 0.3 * _randn(g, c), "be": 0.2 * _randn(g, c)}


def mlp_inputs(c, b, t, m):
    """``x``: the plain MLP's input; ``res``: its residual and the un-normalised input of the LN entries (mean m)."""
    return {"x": shifted_input(c, b, t, 0, 8500), "res": shifted_input(c, b, t, m, 8600)}


def mlp_expected(c, b, t, m, dtype):
    p = {k: v.to(dtype) for k, v in mlp_params(c).items()}
    d = {k: v.to(dtype) for k, v in mlp_inputs(c, b, t, m).items()}
    return {"mlp": R.mlp(d["x"], p["w1"], p["b1"], p["w2"], p["b2"], p["sc"], d["res"]),
            "ln_mlp": R.ln_mlp(d["res"], p["g"], p["be"], 1e-5, p["w1"], p["b1"], p["w2"], p["b2"], p["sc"])}


# ---- transformer.hip: otp_ln_channel ---------------------------------------------------------------------------------------------
def wave_split(c):
    """Channels over the four waves of the split kernels: cw = ceil(C / 4) per wave, the last non-empty wave's count, empty waves."""
    cw = (c + 3) // 4
    used = -(-c // cw)
    return f"cw={cw} lastwave={c - (used - 1) * cw} empty={4 - used}"


def ln_width_branch(c):
    """otp_ln_channel: (kernel and its split of the channels, tokens per workgroup)."""
    if c <= 17:
        return f"reg17 c={c} masked={17 - c}", 256
    if c <= 136:
        return "split34 " + wave_split(c), 64
    if c <= 204:
        return "split51 " + wave_split(c), 64
    return "generic", 256


def tile_branch(t, tile):
    return f"tiles={-(-t // tile)} last={(t - 1) % tile + 1}"


# (C, branch) and (tokens per workgroup, T, branch); a case is a width with a length on the width's tile
LN_WIDTHS = [
    (1, "reg17 c=1 masked=16"),
    (5, "reg17 c=5 masked=12"),
    (17, "reg17 c=17 masked=0"),
    (18, "split34 cw=5 lastwave=3 empty=0"),
    (133, "split34 cw=34 lastwave=31 empty=0"),
    (136, "split34 cw=34 lastwave=34 empty=0"),
    (137, "split51 cw=35 lastwave=32 empty=0"),
    (204, "split51 cw=51 lastwave=51 empty=0"),
    (205, "generic"),
    (260, "generic"),
]
LN_T = [
    (64, 1, "tiles=1 last=1"),
    (64, 63, "tiles=1 last=63"),
    (64, 64, "tiles=1 last=64"),
    (64, 65, "tiles=2 last=1"),
    (64, 257, "tiles=5 last=1"),
    (256, 1, "tiles=1 last=1"),
    (256, 63, "tiles=1 last=63"),
    (256, 64, "tiles=1 last=64"),
    (256, 65, "tiles=1 last=65"),
    (256, 257, "tiles=2 last=1"),
]
# x = 32 + N(0, 1): one case per kernel, on a ragged length; the float32 yardstick is off by 1.0e-5, 7.4e-6, 8.0e-6, 1.1e-5
# there (cap 2.0e-4)
LN_SHIFTED = [(5, 65), (136, 65), (204, 65), (260, 257)]
LN_CASES = ([(c, t, 0, f"{wb} {tb}") for c, wb in LN_WIDTHS for tile, t, tb in LN_T if tile == ln_width_branch(c)[1]]
            + [(c, t, M, f"{wb} {tb}") for c, wb in LN_WIDTHS for tile, t, tb in LN_T
               if tile == ln_width_branch(c)[1] and (c, t) in LN_SHIFTED])


def ln_expected(c, b, t, m, dtype):
    d = ln_inputs(b, c, t, m)
    return [R.layer_norm(d["x"].to(dtype), d["gamma"].to(dtype), d["beta"].to(dtype))]


# ---- transformer.hip: otp_dwconv_ln3 ---------------------------------------------------------------------------------------------
def dw_width_branch(c):
    """otp_dwconv_ln3: (kernel and its split of the channels, output tokens per workgroup)."""
    if c <= 20:
        return "split5 " + wave_split(c), 64
    if c <= 136:
        return "split34 " + wave_split(c), 64
    if c <= 204:
        return "split51 " + wave_split(c), 64
    return "generic", 256


def dw_edge_branch(t, stride, tile):
    """Output length, its tiles, and the taps that are padding: the left one of output 0 always, the right one of the last output
    when ``(To - 1) stride + 1 >= T`` (never for an even T under stride 2)."""
    to = R.dwconv3_out_len(t, stride)
    rpad = int((to - 1) * stride + 1 >= t)
    return f"s={stride} T={t} To={to} {tile_branch(to, tile)} lpad=1 rpad={rpad}"


# (C, branch) and (output tokens per workgroup, stride, T, branch)
DW_WIDTHS = [
    (1, "split5 cw=1 lastwave=1 empty=3"),
    (5, "split5 cw=2 lastwave=1 empty=1"),
    (20, "split5 cw=5 lastwave=5 empty=0"),
    (21, "split34 cw=6 lastwave=3 empty=0"),
    (136, "split34 cw=34 lastwave=34 empty=0"),
    (137, "split51 cw=35 lastwave=32 empty=0"),
    (204, "split51 cw=51 lastwave=51 empty=0"),
    (205, "generic"),
    (260, "generic"),
]
DW_EDGES = [
    (64, 1, 1, "s=1 T=1 To=1 tiles=1 last=1 lpad=1 rpad=1"),
    (64, 1, 2, "s=1 T=2 To=2 tiles=1 last=2 lpad=1 rpad=1"),
    (64, 1, 3, "s=1 T=3 To=3 tiles=1 last=3 lpad=1 rpad=1"),
    (64, 1, 63, "s=1 T=63 To=63 tiles=1 last=63 lpad=1 rpad=1"),
    (64, 1, 64, "s=1 T=64 To=64 tiles=1 last=64 lpad=1 rpad=1"),
    (64, 1, 65, "s=1 T=65 To=65 tiles=2 last=1 lpad=1 rpad=1"),
    (64, 1, 127, "s=1 T=127 To=127 tiles=2 last=63 lpad=1 rpad=1"),
    (64, 1, 128, "s=1 T=128 To=128 tiles=2 last=64 lpad=1 rpad=1"),
    (64, 1, 129, "s=1 T=129 To=129 tiles=3 last=1 lpad=1 rpad=1"),
    (64, 1, 250, "s=1 T=250 To=250 tiles=4 last=58 lpad=1 rpad=1"),
    (64, 2, 1, "s=2 T=1 To=1 tiles=1 last=1 lpad=1 rpad=1"),
    (64, 2, 2, "s=2 T=2 To=1 tiles=1 last=1 lpad=1 rpad=0"),
    (64, 2, 3, "s=2 T=3 To=2 tiles=1 last=2 lpad=1 rpad=1"),
    (64, 2, 63, "s=2 T=63 To=32 tiles=1 last=32 lpad=1 rpad=1"),
    (64, 2, 64, "s=2 T=64 To=32 tiles=1 last=32 lpad=1 rpad=0"),
    (64, 2, 65, "s=2 T=65 To=33 tiles=1 last=33 lpad=1 rpad=1"),
    (64, 2, 127, "s=2 T=127 To=64 tiles=1 last=64 lpad=1 rpad=1"),
    (64, 2, 128, "s=2 T=128 To=64 tiles=1 last=64 lpad=1 rpad=0"),
    (64, 2, 129, "s=2 T=129 To=65 tiles=2 last=1 lpad=1 rpad=1"),
    (64, 2, 250, "s=2 T=250 To=125 tiles=2 last=61 lpad=1 rpad=0"),
    (256, 1, 1, "s=1 T=1 To=1 tiles=1 last=1 lpad=1 rpad=1"),
    (256, 1, 2, "s=1 T=2 To=2 tiles=1 last=2 lpad=1 rpad=1"),
    (256, 1, 3, "s=1 T=3 To=3 tiles=1 last=3 lpad=1 rpad=1"),
    (256, 1, 63, "s=1 T=63 To=63 tiles=1 last=63 lpad=1 rpad=1"),
    (256, 1, 64, "s=1 T=64 To=64 tiles=1 last=64 lpad=1 rpad=1"),
    (256, 1, 65, "s=1 T=65 To=65 tiles=1 last=65 lpad=1 rpad=1"),
    (256, 1, 127, "s=1 T=127 To=127 tiles=1 last=127 lpad=1 rpad=1"),
    (256, 1, 128, "s=1 T=128 To=128 tiles=1 last=128 lpad=1 rpad=1"),
    (256, 1, 129, "s=1 T=129 To=129 tiles=1 last=129 lpad=1 rpad=1"),
    (256, 1, 250, "s=1 T=250 To=250 tiles=1 last=250 lpad=1 rpad=1"),
    (256, 2, 1, "s=2 T=1 To=1 tiles=1 last=1 lpad=1 rpad=1"),
    (256, 2, 2, "s=2 T=2 To=1 tiles=1 last=1 lpad=1 rpad=0"),
    (256, 2, 3, "s=2 T=3 To=2 tiles=1 last=2 lpad=1 rpad=1"),
    (256, 2, 63, "s=2 T=63 To=32 tiles=1 last=32 lpad=1 rpad=1"),
    (256, 2, 64, "s=2 T=64 To=32 tiles=1 last=32 lpad=1 rpad=0"),
    (256, 2, 65, "s=2 T=65 To=33 tiles=1 last=33 lpad=1 rpad=1"),
    (256, 2, 127, "s=2 T=127 To=64 tiles=1 last=64 lpad=1 rpad=1"),
    (256, 2, 128, "s=2 T=128 To=64 tiles=1 last=64 lpad=1 rpad=0"),
    (256, 2, 129, "s=2 T=129 To=65 tiles=1 last=65 lpad=1 rpad=1"),
    (256, 2, 250, "s=2 T=250 To=125 tiles=1 last=125 lpad=1 rpad=0"),
    (256, 1, 257, "s=1 T=257 To=257 tiles=2 last=1 lpad=1 rpad=1"),
]
DW_FAMILIES = ["split5", "split34", "split51", "generic"]
# x = 32 + N(0, 1): one case per kernel, both strides between them; the float32 yardstick is off by at most 5.3e-5 (cap 2.0e-4)
DW_SHIFTED = [(5, 1, 65), (136, 2, 65), (204, 1, 129), (260, 2, 250)]


def _dw_cases():
    """Every (kernel, stride, T) once; the widths of a kernel take turns along T so that every width appears."""
    cases = []
    for fam in DW_FAMILIES:
        widths = [(c, wb) for c, wb in DW_WIDTHS if wb.split()[0] == fam]
        edges = [e for e in DW_EDGES if e[0] == dw_width_branch(widths[0][0])[1]]
        for i, (_, stride, t, eb) in enumerate(edges):
            c, wb = widths[i % len(widths)]
            cases.append((c, stride, t, 0, f"{wb} {eb}"))
    by_key = {(c, s, t): br for c, s, t, _, br in cases}
    for c, s, t in DW_SHIFTED:
        wb = dict(DW_WIDTHS)[c]
        eb = [e[3] for e in DW_EDGES if e[:3] == (dw_width_branch(c)[1], s, t)][0]
        cases.append((c, s, t, M, by_key.get((c, s, t), f"{wb} {eb}")))
    return cases


DW_CASES = _dw_cases()


def dwln_expected(c, b, t, stride, m, dtype):
    p, x = dw_params(c, bool(m)), shifted_input(c, b, t, m, 8700)
    cast = lambda vs: [v.to(dtype) for v in vs]                                        # noqa: E731
    return R.dwconv_ln3(x.to(dtype), cast(p["dws"]), cast(p["gs"]), cast(p["be"]), stride)


# ---- flowenc.hip: otp_flow_front, otp_flow_back ----------------------------------------------------------------------------------
FLOW_C = 17


def flow_hidden_branch(hidden):
    """flow_back_kernel: ``for (m = wave; m < H; m += 4)`` - hidden units per wave and the waves with none."""
    units = [len(range(w, hidden, 4)) for w in range(4)]
    return f"H={hidden} units={'/'.join(map(str, units))} idle_waves={units.count(0)}"


# (T, branch) on the 64-token workgroups of both kernels, (hidden, branch)
FLOW_T = [
    (1, "tiles=1 last=1"),
    (2, "tiles=1 last=2"),
    (63, "tiles=1 last=63"),
    (64, "tiles=1 last=64"),
    (65, "tiles=2 last=1"),
    (333, "tiles=6 last=13"),
]
FLOW_H = [
    (1, "H=1 units=1/0/0/0 idle_waves=3"),
    (3, "H=3 units=1/1/1/0 idle_waves=1"),
    (4, "H=4 units=1/1/1/1 idle_waves=0"),
    (5, "H=5 units=2/1/1/1 idle_waves=0"),
    (68, "H=68 units=17/17/17/17 idle_waves=0"),
]
# (T, mean offset m, branch) / (hidden, T, m, branch); at m = 32 the float32 yardstick is off by 1.9e-5 (front, cap 1.2e-4)
# and 5.4e-6 (back, cap 1.1e-3)
FLOW_FRONT_CASES = [(t, 0, br) for t, br in FLOW_T] + [(t, M, br) for t, br in FLOW_T if t == 65]
FLOW_BACK_CASES = ([(68, t, 0, f"{dict(FLOW_H)[68]} {br}") for t, br in FLOW_T]
                   + [(h, t, 0, f"{hb} {br}") for h, hb in FLOW_H if h != 68 for t, br in FLOW_T if t == 65]
                   + [(h, t, M, f"{hb} {br}") for h, hb in FLOW_H if h in (5, 68) for t, br in FLOW_T if t == 65])


@functools.lru_cache(maxsize=None)
def flow_block(hidden=4 * FLOW_C):
    """A seeded flow-encoder TransformerBlock whose MLP is ``hidden`` wide (the reference's is 4 C = 68)."""
    from otpose_amd import modules
    from otpose_amd import synthetic
    blk = modules.TransformerBlock(FLOW_C, 1, (1, 1), proj_pdrop=0.1, path_pdrop=0.1)
    if hidden != 4 * FLOW_C:
        blk.mlp[0], blk.mlp[3] = torch.nn.Conv1d(FLOW_C, hidden, 1), torch.nn.Conv1d(hidden, FLOW_C, 1)
    return synthetic.fill_synthetic_(blk, 12).eval()


def flow_front_block(blk):
    """The parameter block of otp_flow_front in the layout include/otpose_hip.h documents (ops.pack_flow_front builds the same)."""
    a = blk.attn
    f = lambda t: t.detach().float().reshape(-1)                                       # noqa: E731
    parts = [f(blk.ln1.weight), f(blk.ln1.bias)]
    for conv, norm, proj in ((a.query_conv, a.query_norm, a.query), (a.key_conv, a.key_norm, a.key),
                             (a.value_conv, a.value_norm, a.value)):
        parts += [f(conv.weight), f(norm.weight), f(norm.bias), f(proj.weight), f(proj.bias)]
    return torch.cat(parts).contiguous()


def flow_back_block(blk):
    """The parameter block of otp_flow_back: drop-path scales folded into the projection / down-projection rows and biases, W_2
    transposed to (hidden, C) (ops.pack_flow_back builds the same)."""
    a, c, hid = blk.attn, FLOW_C, blk.mlp[0].out_channels
    d = lambda t: t.detach().float()                                                   # noqa: E731
    sa, sm = d(blk.drop_path_attn.scale).reshape(-1), d(blk.drop_path_mlp.scale).reshape(-1)
    wp = d(a.proj.weight).reshape(c, c) * sa[:, None]
    w2 = d(blk.mlp[3].weight).reshape(c, hid) * sm[:, None]
    return torch.cat([wp.reshape(-1), d(a.proj.bias) * sa, d(blk.ln2.weight).reshape(-1), d(blk.ln2.bias).reshape(-1),
                      d(blk.mlp[0].weight).reshape(-1), d(blk.mlp[0].bias), w2.t().contiguous().reshape(-1),
                      d(blk.mlp[3].bias) * sm]).contiguous()


def flow_inputs(b, t, m):
    return {"x": shifted_input(FLOW_C, b, t, m, 8800), "att": shifted_input(FLOW_C, b, t, 0, 8900)}


def flow_expected(kind, hidden, b, t, m, dtype):
    blk, d = flow_block(hidden), flow_inputs(b, t, m)
    if kind == "front":
        return R.flow_front(d["x"].to(dtype), flow_front_block(blk).to(dtype), blk.ln1.eps)
    return [R.flow_back(d["x"].to(dtype), d["att"].to(dtype), flow_back_block(blk).to(dtype), hidden, blk.ln2.eps)]


# ---- half-operand twins: otp_dense_h1, otp_qkv_front_h1, otp_ln_mlp_h1 ---------------------------------------------------------------
H1_CASES = [(c, t) for c in (136, 204) for t in (2, 126, 130)]
H1_BATCH = 3
