"""`otpose_amd.engine.Routes`: the engines' `OTPOSE_*` switches, read once.  Every name keeps its spelling, default and meaning."""
import dataclasses
import os

import pytest

from otpose_amd.engine import Routes

# switch -> (field, default, a non-default setting, the field's value under it)
SWITCHES = {
    "OTPOSE_HIP_GRAPH": ("use_graph", True, "0", False),
    "OTPOSE_WINOGRAD": ("use_winograd", True, "0", False),
    "OTPOSE_CONV_MATH": ("use_x3", True, "f32", False),
    "OTPOSE_DCN_FUSED": ("use_dcn_fused", True, "0", False),
    "OTPOSE_S8": ("use_s8", True, "0", False),
    "OTPOSE_FLOW_FUSED": ("use_flow_fused", True, "0", False),
    "OTPOSE_SMALL_CONV": ("use_small_conv", True, "0", False),
    "OTPOSE_FUSED_MLP": ("use_fused_mlp", True, "0", False),
    "OTPOSE_FUSE_SHORTCUT": ("fuse_shortcut", True, "0", False),
    "OTPOSE_FUSE_UPSAMPLE": ("fuse_upsample", True, "0", False),
    "OTPOSE_DENSE_CC": ("use_dense_cc", True, "0", False),
    "OTPOSE_QKV_FRONT": ("use_qkv_front", True, "0", False),
    "OTPOSE_POINTX": ("use_pointx", True, "0", False),
    "OTPOSE_POINTX_FUSE": ("pointx_fuse", True, "0", False),
    "OTPOSE_POINTX_ANY": ("pointx_any", False, "1", True),
    "OTPOSE_STREAMS": ("multi_stream", True, "0", False),
    "OTPOSE_F32_TAIL": ("f32_tail", 0, "2", 2),
    "OTPOSE_H16_TAIL": ("h16_tail", True, "0", False),
    "OTPOSE_RANGE_CHECK": ("range_check", "defer", "sync", "sync"),
    "OTPOSE_S8_RESIDUAL": ("s8_residual", True, "0", False),
    "OTPOSE_S8_LAZY_NCHW": ("s8_lazy_nchw", True, "0", False),
    "OTPOSE_S8_STRIDE2": ("s8_stride2", True, "0", False),
    "OTPOSE_T1_S8": ("t1_s8", True, "0", False),
    "OTPOSE_L1_S8": ("l1_s8", True, "0", False),
    "OTPOSE_L1_PAIR": ("l1_pair", True, "0", False),
    "OTPOSE_STEM_X3": ("stem_x3", True, "0", False),
    "OTPOSE_CHAIN_MODULES": ("chain_modules", True, "0", False),
    "OTPOSE_UP_ANY_WIDTH": ("up_any_width", True, "0", False),
    "OTPOSE_CONV_LOG": ("conv_log", False, "1", True),
    "OTPOSE_POISON": ("poison", None, "3:7", (3, 7)),
    "OTPOSE_TE_SERIAL": ("te_serial", False, "1", True),
}
# fields that follow another switch: OTPOSE_CONV_MATH=f32 leaves only the exact-fp32 kernels
GATED = {"OTPOSE_CONV_MATH": {"use_dcn_fused": False, "use_s8": False, "use_pointx": False, "f32_tail": 0}}


@pytest.fixture
def clean_env(monkeypatch):
    for name in [k for k in os.environ if k.startswith("OTPOSE_")]:
        monkeypatch.delenv(name)
    return monkeypatch


def test_every_field_has_its_switch_and_default(clean_env):
    r = Routes.from_env()
    assert {f.name for f in dataclasses.fields(Routes)} == {field for field, *_ in SWITCHES.values()}
    for name, (field, default, _, _) in SWITCHES.items():
        assert getattr(r, field) == default and type(getattr(r, field)) is type(default), name
    assert r == Routes()
    assert r.lazy_nchw


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_a_switch_flips_its_own_field_and_the_fields_gated_on_it(clean_env, name):
    field, _, setting, value = SWITCHES[name]
    base = dataclasses.asdict(Routes.from_env())
    clean_env.setenv(name, setting)
    got = dataclasses.asdict(Routes.from_env())
    assert got == {**base, field: value, **GATED.get(name, {})}


def test_exact_fp32_math_gates_the_split_product_routes(clean_env):
    clean_env.setenv("OTPOSE_CONV_MATH", "f32")
    clean_env.setenv("OTPOSE_F32_TAIL", "2")
    r = Routes.from_env()
    assert not (r.use_x3 or r.use_dcn_fused or r.use_s8 or r.use_pointx) and r.f32_tail == 0


def test_f32_tail_reads_as_a_count(clean_env):
    clean_env.setenv("OTPOSE_F32_TAIL", "2")
    assert Routes.from_env().f32_tail == 2


def test_lazy_nchw_needs_the_s8_residual(clean_env):
    clean_env.setenv("OTPOSE_S8_RESIDUAL", "0")
    assert not Routes.from_env().lazy_nchw
    clean_env.delenv("OTPOSE_S8_RESIDUAL")
    clean_env.setenv("OTPOSE_S8_LAZY_NCHW", "0")
    assert not Routes.from_env().lazy_nchw
