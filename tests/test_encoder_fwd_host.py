"""tests/encoder_fwd_ref.py and tests/encoder_fwd_cases.py pinned on the CPU (no GPU, no hip.lib()): every case's branch text
derived again from its numbers by the host rule or kernel loop it restates; every branch those rules can produce at the listed
sizes named by a case; the restatements against oracle/otpose_oracle.py run on the float64 state dict of a seeded
modules.TransformerBlock (the modules hold parameters and compute nothing themselves), to 1e-12; the float32 yardstick inside
its cap on every case, the shifted-mean ones included, and the shift the largest of LN_OFFSETS at which it still is - so that
tests/test_gpu_encoder_fwd.py keeps reaching every tile edge, route and width it was written for."""
import pytest
import torch
import torch.nn.functional as F

from oracle import otpose_oracle as O
from tests import encoder_fwd_cases as C
from tests import encoder_fwd_ref as R
from tests import reductions_cases as K

D = torch.float64


def _eq(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---- branch text from the numbers ------------------------------------------------------------------------------------------
def test_dense_and_front_branches():
    for t, branch in C.DENSE_T:
        assert C.dense_branch(t) == branch
        assert all(C.dense_supported(e, c, t) for e, c in C.DENSE_ENTRIES)
    for t, _, branch in C.FRONT_T:
        assert C.front_branch(t) == branch and branch.startswith(C.dense_branch(t))
    assert not C.dense_supported("cc", 204, 128) and not C.dense_supported("x3", 136, 127)


def test_dense_cases_cover_the_launches():
    """Every entry at every T of the issue, launches of 1, 2 and 3 problems with and without residual and the mixed one."""
    assert [t for t, _ in C.DENSE_T] == [2, 30, 32, 34, 126, 128, 130, 258]
    for e, c in C.DENSE_ENTRIES:
        mine = [k for k in C.DENSE_CASES if k[:2] == (e, c)]
        assert {k[2] for k in mine} == {t for t, _ in C.DENSE_T}
        assert {k[3] for k in mine} == set(C.DENSE_PATTERNS)
    assert {(e, c) for e, c in C.DENSE_ENTRIES} == {("cc", 136), ("x3", 136), ("x3", 204), ("bf16p", 136), ("bf16p", 204)}
    # the clamp where nearly every lane takes it, a full tile, one live pair in a second and third workgroup
    names = [b for _, b in C.DENSE_T]
    assert any("tiles=1 last=2 clamped=252" in n for n in names) and any("clamped=0" in n for n in names)
    assert any("tiles=2 last=2" in n for n in names) and any("tiles=3 last=2" in n for n in names)
    front = [b for _, _, b in C.FRONT_T]
    assert any("l_false=256 r_false=256" in n for n in front)                   # T = 2: no lane has a neighbour
    assert any("l_false=4 r_false=4" in n for n in front)                       # only the two ends of the sequence
    assert {m for _, m, _ in C.FRONT_T} == {0, C.M}


@pytest.mark.parametrize("case", C.MLP_CASES)
def test_mlp_case_branch(case):
    kernel, c, t, nt1, bal, m, branch = case
    assert c in C.MLP_WIDTHS[kernel] and t % 2 == 0
    for b in C.BATCHES:
        assert C.mlp_branch(kernel, c, b, t, nt1, bal) == branch


def test_mlp_cases_cover_the_forms():
    forms = {" ".join(k[-1].split()[:2]) for k in C.MLP_CASES}
    assert forms == {"mlp nt2x4", "mlp balanced", "mlpx nt1x8", "mlpx nt2x8", "mlpx balanced", "mlpx204 nt1x8"}
    plain = [k for k in C.MLP_CASES if not k[5]]
    by = lambda kernel, c, nt1, bal: {k[2] for k in plain if (k[0], k[1], k[3], k[4]) == (kernel, c, nt1, bal)}   # noqa: E731
    for kernel in ("fused", "x3"):
        assert by(kernel, 136, None, None) >= {2, 14, 16, 18, 126, 128, 130}
        assert by(kernel, 136, None, "2") == {432, 864}
    assert by("fused", 136, None, None) >= {30, 32, 34}                          # the 32-token wave edge of mlp.hip: idle_waves = 2
    assert any(k[0] == "fused" and "idle_waves=2" in k[-1] for k in plain)
    assert by("x3", 136, "0", None) == {30, 32, 34, 254, 256, 258}
    assert by("x3", 204, None, None) == {2, 126, 130}
    # every form also runs its LayerNorm on a shifted input
    assert {" ".join(k[-1].split()[:2]) for k in C.MLP_CASES if k[5]} == forms
    # the automatic rule (no environment) stays off the balanced form at these sizes and takes it from B * T / 432 >= 192
    assert "balanced" not in C.mlp_branch("fused", 136, 3, 432) and "balanced" in C.mlp_branch("fused", 136, 192, 432)
    assert "balanced" in C.mlp_branch("x3", 136, 96, 864, "0") and "nt1x8" in C.mlp_branch("x3", 136, 96, 864)
    assert "nt2x8" in C.mlp_branch("x3", 136, 3, 430, None, "2") and "balanced" not in C.mlp_branch("x3", 136, 192, 432, "0", "0")


def test_ln_channel_branches_and_coverage():
    for c, branch in C.LN_WIDTHS:
        assert C.ln_width_branch(c)[0] == branch
    for tile, t, branch in C.LN_T:
        assert C.tile_branch(t, tile) == branch
    assert [c for c, _ in C.LN_WIDTHS] == [1, 5, 17, 18, 133, 136, 137, 204, 205, 260]
    lengths = [1, 63, 64, 65, 257]
    assert sorted(t for tile, t, _ in C.LN_T if tile == 64) == lengths == sorted(t for tile, t, _ in C.LN_T if tile == 256)
    # every branch the rule can produce for these widths and lengths is named by a case, C = 17, 136, 204 and the generic widths
    want = {f"{C.ln_width_branch(c)[0]} {C.tile_branch(t, C.ln_width_branch(c)[1])}" for c, _ in C.LN_WIDTHS for t in lengths}
    have = {k[-1] for k in C.LN_CASES}
    assert want == have, want ^ have
    assert {k[-1].split()[0] for k in C.LN_CASES} == {"reg17", "split34", "split51", "generic"}
    assert {k[-1].split()[0] for k in C.LN_CASES if k[2]} == {"reg17", "split34", "split51", "generic"}
    for c in (17, 136, 204, 205, 260):
        assert {k[1] for k in C.LN_CASES if k[0] == c} == set(lengths)
    assert C.ln_width_branch(17)[0].startswith("reg17") and C.ln_width_branch(18)[0].startswith("split34")
    assert C.ln_width_branch(136)[0].startswith("split34") and C.ln_width_branch(137)[0].startswith("split51")
    assert C.ln_width_branch(204)[0].startswith("split51") and C.ln_width_branch(205)[0] == "generic"


def test_dwconv_ln3_branches_and_coverage():
    for c, branch in C.DW_WIDTHS:
        assert C.dw_width_branch(c)[0] == branch
    for tile, stride, t, branch in C.DW_EDGES:
        assert C.dw_edge_branch(t, stride, tile) == branch
    assert [c for c, _ in C.DW_WIDTHS] == [1, 5, 20, 21, 136, 137, 204, 205, 260]
    lengths = {1, 2, 3, 63, 64, 65, 127, 128, 129, 250}
    # every (kernel, stride, length) once, every width somewhere, nothing the rule can produce left out
    want = {(fam, s, t) for fam in C.DW_FAMILIES for s in (1, 2) for t in lengths} | {("generic", 1, 257)}
    plain = [k for k in C.DW_CASES if not k[3]]
    have = [(k[-1].split()[0], k[1], k[2]) for k in plain]
    assert len(have) == len(set(have)) and set(have) == want, set(have) ^ want
    assert {k[0] for k in C.DW_CASES} == {c for c, _ in C.DW_WIDTHS}
    for k in C.DW_CASES:
        c, s, t, m, branch = k
        wb, tile = C.dw_width_branch(c)
        assert branch == f"{wb} {C.dw_edge_branch(t, s, tile)}"
    assert {(k[-1].split()[0], k[1]) for k in C.DW_CASES if k[3]} >= {("split5", 1), ("split34", 2), ("split51", 1), ("generic", 2)}
    names = [k[-1] for k in C.DW_CASES]
    for fam in C.DW_FAMILIES:                            # both neighbours padding; odd T under stride 2; a ragged second tile
        assert any(n.startswith(fam) and " T=1 " in n for n in names)
        assert any(n.startswith(fam) and "s=2 T=129 " in n for n in names)
        assert any(n.startswith(fam) and "tiles=2 last=1" in n for n in names)
    assert any("empty=3" in n for n in names) and any("empty=1" in n for n in names)


def test_flow_branches_and_coverage():
    for t, branch in C.FLOW_T:
        assert C.tile_branch(t, 64) == branch
    for h, branch in C.FLOW_H:
        assert C.flow_hidden_branch(h) == branch
    assert [t for t, _ in C.FLOW_T] == [1, 2, 63, 64, 65, 333] and [h for h, _ in C.FLOW_H] == [1, 3, 4, 5, 68]
    assert {k[0] for k in C.FLOW_FRONT_CASES} == {t for t, _ in C.FLOW_T} == {k[1] for k in C.FLOW_BACK_CASES if k[0] == 68}
    assert {k[0] for k in C.FLOW_BACK_CASES} == {1, 3, 4, 5, 68}
    names = [k[-1] for k in C.FLOW_BACK_CASES]
    assert any("idle_waves=3" in n for n in names) and any("idle_waves=1" in n for n in names)      # H < 4
    assert any("units=2/1/1/1" in n for n in names)                                                  # H % 4 != 0
    assert any(k[1] for k in C.FLOW_FRONT_CASES) and {k[0] for k in C.FLOW_BACK_CASES if k[2]} == {5, 68}
    assert C.H1_CASES == [(c, t) for c in (136, 204) for t in (2, 126, 130)]


# ---- the restatements against the oracle on a seeded module's parameters ----------------------------------------------------
def _block(c, heads, stride=1):
    from otpose_amd import modules, synthetic
    blk = synthetic.fill_synthetic_(modules.TransformerBlock(c, heads, (stride, stride), proj_pdrop=0.1, path_pdrop=0.1), 5).eval()
    assert not blk.training
    return blk, {"b." + k: v.detach().to(D) for k, v in blk.state_dict().items()}


def _front_of(sd, x, stride):
    names = ("query", "key", "value")
    return ([sd[f"b.attn.{n}_conv.weight"] for n in names], [sd[f"b.attn.{n}_norm.weight"] for n in names],
            [sd[f"b.attn.{n}_norm.bias"] for n in names], [sd[f"b.attn.{n}.weight"] for n in names],
            [sd[f"b.attn.{n}.bias"] for n in names])


@pytest.mark.parametrize("c,heads,t", [(8, 2, 11), (17, 1, 6), (12, 3, 1)])
def test_restatements_agree_with_the_transformer_block(c, heads, t):
    """ln1 -> q/k/v front end -> channel attention -> proj + residual -> ln2 + MLP + residual, piece by piece from the
    restatements, against the oracle's TransformerBlock on the same state dict; the intermediate LayerNorm against
    oracle.channel_layernorm."""
    blk, sd = _block(c, heads)
    assert isinstance(blk.attn, __import__("otpose_amd.modules", fromlist=["MaskedMHCA"]).MaskedMHCA)
    x = torch.randn(3, c, t, dtype=D, generator=K.gen(41))
    ln1 = R.layer_norm(x, sd["b.ln1.weight"], sd["b.ln1.bias"], blk.ln1.eps)
    _eq(ln1, O.channel_layernorm(sd, "b.ln1", x))
    dws, gs, be, ws, bs = _front_of(sd, x, 1)
    q, k, v = R.qkv_front(ln1, dws, gs, be, ws, bs, blk.attn.query_norm.eps)
    att = R.chan_attn_expr(q, k, v, heads, blk.attn.scale)
    _eq(R.pointwise(att, sd["b.attn.proj.weight"], sd["b.attn.proj.bias"]), O.masked_mhca(sd, "b.attn", ln1, heads, 1))
    y = R.pointwise(att, sd["b.attn.proj.weight"], sd["b.attn.proj.bias"], sd["b.drop_path_attn.scale"], x)
    out = R.ln_mlp(y, sd["b.ln2.weight"], sd["b.ln2.bias"], blk.ln2.eps, sd["b.mlp.0.weight"], sd["b.mlp.0.bias"],
                   sd["b.mlp.3.weight"], sd["b.mlp.3.bias"], sd["b.drop_path_mlp.scale"])
    _eq(out, O.transformer_block(sd, "b", x, heads, 1))
    # the plain MLP entry is the same line with the normalised tensor handed in
    _eq(R.mlp(O.channel_layernorm(sd, "b.ln2", y), sd["b.mlp.0.weight"], sd["b.mlp.0.bias"], sd["b.mlp.3.weight"],
              sd["b.mlp.3.bias"], sd["b.drop_path_mlp.scale"], y), out)


@pytest.mark.parametrize("t,stride", [(1, 1), (1, 2), (2, 2), (9, 1), (9, 2), (10, 2)])
def test_dwconv_ln3_restatement(t, stride):
    blk, sd = _block(8, 2, stride)
    x = torch.randn(2, 8, t, dtype=D, generator=K.gen(42))
    dws, gs, be, _, _ = _front_of(sd, x, stride)
    for i, name in enumerate(("query", "key", "value")):
        ref = O.channel_layernorm(sd, f"b.attn.{name}_norm", F.conv1d(x, dws[i], None, stride, 1, 1, 8))
        _eq(R.dwconv_ln3(x, dws, gs, be, stride)[i], ref)


@pytest.mark.parametrize("hidden", [68, 5, 1])
def test_flow_restatements_from_the_parameter_blocks(hidden):
    """flow_front / flow_back read the blocks ops.pack_flow_front / pack_flow_back lay out; from the float64 blocks of a seeded
    17-channel block they give the oracle's q / k / v path and block output (the blocks themselves are float32 roundings, so the
    state dict is rebuilt from them)."""
    blk = C.flow_block(hidden)
    assert blk.mlp[0].out_channels == hidden and not blk.training
    sd = {"b." + k: v.detach().to(D) for k, v in blk.state_dict().items()}
    x = torch.randn(3, 17, 7, dtype=D, generator=K.gen(43))
    front, back = C.flow_front_block(blk).to(D), C.flow_back_block(blk).to(D)
    ln1 = O.channel_layernorm(sd, "b.ln1", x)
    dws, gs, be, ws, bs = _front_of(sd, x, 1)
    q, k, v = R.flow_front(x, front, blk.ln1.eps)
    for got, ref in zip((q, k, v), R.qkv_front(ln1, dws, gs, be, ws, bs)):
        _eq(got, ref)
    att = R.chan_attn_expr(q, k, v, 1, blk.attn.scale)
    _eq(R.flow_back(x, att, back, hidden, blk.ln2.eps), O.transformer_block(sd, "b", x, 1, 1), 1e-7)     # (fp32 fold of the scales)
    # with the scales folded in float64 the block output is the oracle's to 1e-12
    sa, sm = sd["b.drop_path_attn.scale"].reshape(-1), sd["b.drop_path_mlp.scale"].reshape(-1)
    exact = torch.cat([(sd["b.attn.proj.weight"].reshape(17, 17) * sa[:, None]).reshape(-1), sd["b.attn.proj.bias"] * sa,
                       sd["b.ln2.weight"].reshape(-1), sd["b.ln2.bias"].reshape(-1), sd["b.mlp.0.weight"].reshape(-1),
                       sd["b.mlp.0.bias"], (sd["b.mlp.3.weight"].reshape(17, hidden) * sm[:, None]).t().reshape(-1),
                       sd["b.mlp.3.bias"] * sm])
    _eq(R.flow_back(x, att, exact, hidden, blk.ln2.eps), O.transformer_block(sd, "b", x, 1, 1))
    assert float((exact - back).abs().max()) <= 2.0 ** -23 * float(exact.abs().max())


# ---- the float32 yardstick inside its cap, the shifted cases' m the largest that is -----------------------------------------
def _yard(expected, *args):
    """[(error of the float32 restatement against float64, its cap)] per output."""
    ref, yd = expected(*args, D), expected(*args, torch.float32)
    ref, yd = (list(ref.values()), list(yd.values())) if isinstance(ref, dict) else (ref, yd)
    return [(K.max_err(y, r), C.FWD_TOL * max(1.0, float(r.abs().max()))) for y, r in zip(yd, ref)]


def _inside(pairs, what):
    for err, cap in pairs:
        assert err <= cap, f"{what}: the fp32 yardstick is off by {err} (cap {cap})"


def _largest_offset(expected, make_args):
    return max(o for o in C.LN_OFFSETS if all(e <= cap for e, cap in _yard(expected, *make_args(o))))


@pytest.mark.parametrize("b", C.BATCHES)
def test_dense_and_front_yardsticks(b):
    for e, c, t, pattern, _ in C.DENSE_CASES:
        _inside(_yard(C.dense_expected, c, b, t, pattern), f"dense {e} {c} {t}")
    for e, c, t, m, _ in C.FRONT_CASES:
        _inside(_yard(C.front_expected, c, b, t, m), f"front {e} {c} {t} m={m}")
        if m:
            assert m == _largest_offset(C.front_expected, lambda o: (c, b, t, o))


@pytest.mark.parametrize("b", C.BATCHES)
def test_mlp_yardsticks(b):
    for kernel, c, t, _, _, m, _ in C.MLP_CASES:
        _inside(_yard(C.mlp_expected, c, b, t, m), f"mlp {kernel} {c} {t} m={m}")
        if m:
            assert m == _largest_offset(C.mlp_expected, lambda o: (c, b, t, o))


@pytest.mark.parametrize("b", C.BATCHES)
def test_ln_and_dwconv_yardsticks(b):
    for c, t, m, _ in C.LN_CASES:
        _inside(_yard(C.ln_expected, c, b, t, m), f"ln {c} {t} m={m}")
        if m:
            assert m == _largest_offset(C.ln_expected, lambda o: (c, b, t, o))
    for c, s, t, m, _ in C.DW_CASES:
        _inside(_yard(C.dwln_expected, c, b, t, s, m), f"dwconv_ln3 {c} {s} {t} m={m}")
        if m:
            assert m == _largest_offset(C.dwln_expected, lambda o: (c, b, t, s, o))


@pytest.mark.parametrize("b", C.BATCHES)
def test_flow_yardsticks(b):
    for t, m, _ in C.FLOW_FRONT_CASES:
        _inside(_yard(C.flow_expected, "front", 68, b, t, m), f"flow_front {t} m={m}")
        if m:
            assert m == _largest_offset(C.flow_expected, lambda o: ("front", 68, b, t, o))
    for h, t, m, _ in C.FLOW_BACK_CASES:
        _inside(_yard(C.flow_expected, "back", h, b, t, m), f"flow_back {h} {t} m={m}")
        if m:
            assert m == _largest_offset(C.flow_expected, lambda o: ("back", h, b, t, o))


# ---- the shifted cases see what they are there for ------------------------------------------------------------------------------
def _ln_inputs_of(family, args, dtype=D):
    """The tensors the in-kernel LayerNorms of a shifted case normalise (every LayerNorm of the case, in float64)."""
    seen = []
    plain = R.layer_norm
    R.layer_norm = lambda x, g, b, eps=1e-5: (seen.append(x), plain(x, g, b, eps))[1]
    try:
        family(*args, dtype)
    finally:
        R.layer_norm = plain
    return seen


def _one_pass_error(family, args):
    """[(error of the float32 restatement with a one-pass LayerNorm against float64, float32 yardstick error, reference)]."""
    ref, yd = family(*args, D), family(*args, torch.float32)
    plain = R.layer_norm
    R.layer_norm = C.layer_norm_one_pass
    try:
        bad = family(*args, torch.float32)
    finally:
        R.layer_norm = plain
    if isinstance(ref, dict):
        ref, yd, bad = ([v["ln_mlp"]] for v in (ref, yd, bad))
    return [(K.max_err(o, r), K.max_err(y, r), r) for o, y, r in zip(bad, yd, ref)]


def _shifted_cases():
    """(name, expected function, arguments, split-product?) of every case on x = m + N(0, 1), both batch sizes."""
    out = []
    for b in C.BATCHES:
        out += [(f"front {e} {c} {t}", C.front_expected, (c, b, t, m), e != "cc") for e, c, t, m, _ in C.FRONT_CASES if m]
        out += [(f"mlp {k} {c} {t}", C.mlp_expected, (c, b, t, m), k == "x3") for k, c, t, _, _, m, _ in C.MLP_CASES if m]
        out += [(f"ln {c} {t}", C.ln_expected, (c, b, t, m), False) for c, t, m, _ in C.LN_CASES if m]
        out += [(f"dwconv_ln3 {c} {s} {t}", C.dwln_expected, (c, b, t, s, m), False) for c, s, t, m, _ in C.DW_CASES if m]
        out += [(f"flow_front {t}", C.flow_expected, ("front", 68, b, t, m), False) for t, m, _ in C.FLOW_FRONT_CASES if m]
        out += [(f"flow_back {h} {t}", C.flow_expected, ("back", h, b, t, m), False) for h, t, m, _ in C.FLOW_BACK_CASES if m]
    return out


def test_every_shifted_case_puts_the_mean_on_its_layer_norms():
    """What a LayerNorm of the case normalises has a mean many times its spread - for the front ends and dwconv_ln3 that is the
    depthwise conv's output, not x.  Every LayerNorm of the case but flow_front's second (it follows ln1, whose output is
    centred) and, per token, at least 10 for nine tokens in ten (the two ends of a sequence see two taps of three)."""
    for name, family, args, _ in _shifted_cases():
        seen = _ln_inputs_of(family, args)
        assert seen, name
        for x in seen[:1] if name.startswith("flow_front") else seen:
            ratio = x.mean(1).abs() / x.std(1, unbiased=False)
            assert float(ratio.median()) >= 10.0 and float((ratio >= 10.0).double().mean()) >= 0.9, (name, float(ratio.median()))


def test_a_one_pass_layer_norm_misses_the_bound_of_every_shifted_case():
    """E[x^2] - mean^2 in float32, put into the restatement in place of the two-pass form, is further from float64 than the bound
    the GPU test holds the case's kernel to: the exact-fp32 rule, 2e-5 of the range for the split-product front ends, and for the
    split-product LN + MLP the bound on out - res (the bound on the output itself, inflated by the residual's + 32, is only
    about as large as that error and does not decide)."""
    for name, family, args, split in _shifted_cases():
        for i, (bad, yard, ref) in enumerate(_one_pass_error(family, args)):
            if split and family is C.mlp_expected:
                bnd = C.x3_branch_bound(ref, C.mlp_inputs(*args)["res"].to(D))
            else:
                bnd = C.x3_bound(ref) if split else K.bound(yard, ref, C.FWD_TOL)
            assert bad > 2.0 * bnd, f"{name} output {i}: a one-pass LayerNorm is off by {bad}, inside twice the bound {bnd}"


def test_shifted_inputs_have_the_mean_they_name():
    x = C.shifted_input(136, 3, 130, C.M)
    assert abs(float(x.mean()) - C.M) < 0.05 and abs(float(x.std()) - 1.0) < 0.05 and C.M == max(C.LN_OFFSETS)
    assert abs(float(C.ln_inputs(3, 136, 65, C.M)["x"].mean()) - C.M) < 0.05
