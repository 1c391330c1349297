"""The C-ABI library loads on a box without a GPU and exports every symbol include/otpose_hip.h declares."""
import ctypes
import os
import re

import pytest

from otpose_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "otpose_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(otp_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound():
    names = _declared()
    assert "otp_mdcn_forward" in names and "otp_conv2d" in names and len(names) >= 15
    L = hip.lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/otpose_hip.h but not exported"
        assert n in hip.SIGNATURES, f"{n} has no ctypes signature"
    assert sorted(hip.SIGNATURES) == names
    assert L.otp_version() >= 1


def test_bad_arguments_return_error_codes_without_a_gpu():
    L = hip.lib()
    assert L.otp_mdcn_forward(None, None, None, None, None, None, 1, 1, 1, 1, 1, 3, 3, 1, 1, 1, 1, 1, 1.0, 0.0, 0, None) == -1
    assert L.otp_conv2d(None, None, None, None, None, None, None, None, None) == -1
    assert L.otp_chan_attn_workspace(2, 136, 100, 2) > 0
    assert L.otp_loss_workspace(4, 17) > 0


def test_host_side_queries_of_the_temporal_encoder_kernels():
    """Shape predicates, buffer sizes and argument checks of csrc/mlp.hip / dense.hip / the 1x1 wgrad - host code only."""
    L = hip.lib()
    assert L.otp_mlp_fused_supported(136, 544, 6912) == 1
    assert L.otp_mlp_fused_supported(136, 544, 6911) == 0 and L.otp_mlp_fused_supported(17, 68, 6912) == 0
    # 34 hidden blocks of (9 + 9) x 256 fragment floats + 16 biases
    assert L.otp_mlp_fused_weight_bytes(136, 544) == 34 * ((9 + 9) * 256 + 16) * 4
    assert L.otp_mlp_fused_weight_bytes(135, 544) == 0
    assert L.otp_dense_cc_supported(136, 3456) == 1 and L.otp_dense_cc_supported(136, 27) == 0
    assert L.otp_dense_cc_weight_bytes(136) == 9 * 3072 * 4
    assert L.otp_qkv_front_table_bytes(136) == 3 * 136 * 8 * 4
    assert L.otp_ln_channel_backward_workspace(16, 136, 6912) == 2 * 136 * 16 * 108 * 4
    assert L.otp_ln_channel_backward_workspace(16, 150, 6912) == 0            # wider than the register-resident form
    assert L.otp_conv2d_wgrad_workspace(136, 544) >= 96 << 20                 # room for the 1x1 path's per-chunk tiles
    assert L.otp_mlp_fused(None, None, None, None, None, None, 1, 136, 544, 64, None) == -1
    assert L.otp_dense_cc(None, None, None, None, 1, 1, 136, 64, None) == -1
    assert L.otp_qkv_front(None, None, None, None, None, None, None, None, 1, 136, 64, 1e-5, None) == -1
    assert L.otp_loss_joints_mse(None, None, None, None, None, None, 0, 1, 17, 64, 8, 1, 0, None) == -1


_SNIPPET = """
#define OTP_OK 0
#define OTP_ERR_BAD_ARG (-1)     /* a comment after the value */
#define OTP_NOT_AN_INTEGER 1.5f
/* a comment that holds a call otp_foo(1, 2); and a prototype: int otp_ghost(char* p); */
typedef struct otp_toy_desc {
    int a, b;                    /* two ints in one declaration; otp_in_struct(3); */
    float c;
    int d;
} otp_toy_desc;
int otp_nothing(void);
size_t otp_empty();   // int otp_line_comment(int x);
int otp_three_lines(const void* in, void* out,
                    int n, float alpha, double beta,
                    size_t bytes, void* stream);
int otp_pointers(const void* const* lows, void* const* outs, const int* factors, int* out8, const double* sigmas,
                 const otp_toy_desc* desc, unsigned long long seed);
"""


def test_header_parser_maps_each_declaration_shape():
    """hip.parse_header on every shape of declaration include/otpose_hip.h uses (the rule: hip's module docstring)."""
    from ctypes import POINTER, c_double, c_float, c_int, c_size_t, c_ulonglong, c_void_p
    sigs, structs, consts = hip.parse_header(_SNIPPET)
    assert consts == {"OTP_OK": 0, "OTP_ERR_BAD_ARG": -1}
    assert list(structs) == ["otp_toy_desc"]
    toy = structs["otp_toy_desc"]
    assert toy.__name__ == "ToyDesc"
    assert toy._fields_ == [("a", c_int), ("b", c_int), ("c", c_float), ("d", c_int)]
    d = toy(1, 2, 0.5, 4)                                                       # positional construction, declaration order
    assert (d.a, d.b, d.c, d.d) == (1, 2, 0.5, 4)
    assert sorted(sigs) == ["otp_empty", "otp_nothing", "otp_pointers", "otp_three_lines"]     # nothing out of a comment
    assert sigs["otp_nothing"] == (c_int, [])
    assert sigs["otp_empty"] == (c_size_t, [])
    assert sigs["otp_three_lines"] == (c_int, [c_void_p, c_void_p, c_int, c_float, c_double, c_size_t, c_void_p])
    assert sigs["otp_pointers"] == (c_int, [c_void_p, c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_double),
                                            POINTER(toy), c_ulonglong])


@pytest.mark.parametrize("proto, name", [
    ("int otp_bad_text(const void* x, char* name, void* stream);", "otp_bad_text"),
    ("int otp_bad_depth(int** rows);", "otp_bad_depth"),
    ("int otp_bad_struct(const otp_unknown_desc* desc);", "otp_bad_struct"),
    ("int otp_bad_by_value(otp_toy_desc desc);", "otp_bad_by_value"),
    ("int otp_bad_scalar(int n, short m);", "otp_bad_scalar"),
])
def test_header_parser_rejects_an_unmapped_type_and_names_the_prototype(proto, name):
    with pytest.raises(ValueError, match=name):
        hip.parse_header(_SNIPPET + proto)


def test_header_parser_rejects_an_unmapped_struct_field():
    with pytest.raises(ValueError, match="otp_wide_desc"):
        hip.parse_header("typedef struct otp_wide_desc { int n; double x; } otp_wide_desc;")


def test_descriptor_structures_and_constants_come_from_the_header():
    sigs, structs, consts = hip.parse_header(open(os.path.join(ROOT, "include", "otpose_hip.h")).read())
    assert len(hip.SIGNATURES) == len(_declared()) and len(sigs) == len(_declared())
    assert {k: hip.CONSTANTS[k] for k in ("OTP_OK", "OTP_ERR_WORKSPACE", "OTP_DTYPE_F64", "OTP_ACT_GELU", "OTP_S8_F32_NCHW",
                                          "OTP_POSEVAL_JOINTS")} == {"OTP_OK": 0, "OTP_ERR_WORKSPACE": -4, "OTP_DTYPE_F64": 3,
                                                                     "OTP_ACT_GELU": 2, "OTP_S8_F32_NCHW": 2, "OTP_POSEVAL_JOINTS": 15}
    for cls, name in ((hip.ConvDesc, "otp_conv_desc"), (hip.NhwcConvDesc, "otp_nhwc_conv_desc"), (hip.H16ConvDesc, "otp_h16_conv_desc")):
        assert cls._fields_ == structs[name]._fields_ and cls.__name__ == structs[name].__name__
    d = hip.NhwcConvDesc(2, 8, 6, 16, 32, 3, 3, 1, 1, 1, 0)
    assert (d.N, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw, d.stride, d.pad, d.dil, d.out_mode) == (2, 8, 6, 16, 32, 3, 3, 1, 1, 1, 0)
    assert [n for n, _ in hip.ConvDesc._fields_][-2:] == ["out_scale", "res_layout"]
    assert dict(hip.H16ConvDesc._fields_)["out_scale"] is ctypes.c_float
    assert hip.OTP_OK == 0 and sorted(hip._ERRORS) == [-4, -3, -2, -1]
    assert all(hip._ERRORS[hip.CONSTANTS[k]].startswith(k) for k in hip.CONSTANTS if k.startswith("OTP_ERR_"))


def test_pointer_array_parameters_take_none_and_ctypes_arrays():
    """`const void* const*` binds as c_void_p: NULL and (c_void_p * n) arrays reach the library's own argument checks."""
    L = hip.lib()
    assert L.otp_dcn_fused_pack(None, None, None, None, None, 1, 1, None) < 0
    one = [(ctypes.c_void_p * 1)() for _ in range(4)]
    assert L.otp_dense_cc(*one, 1, 0, 136, 64, None) < 0
    assert L.otp_dense_cc(*one, 1, -1, 136, 64, None) < 0
