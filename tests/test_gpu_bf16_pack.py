"""Packed bf16 weights of the NHWC training convolutions (csrc/nhwc_conv.hip): the direct packer (otp_nhwc_conv_pack) and the job-table
packer (otp_nhwc_conv_pack_job + otp_nhwc_conv_pack_batch) must write the same bits on each of the three routes (nhwc_conv_kernel,
csrc/hb.hip's 3x3 window kernel, its pointwise kernel), and the byte count, the statistics row count, the packer and the launch must
agree on which descriptors they take."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN16 = 0x7FC0          # a bfloat16 NaN

# cin, cout, k, stride, pad, dil, h, w, OTPOSE_NHWC_HB (None: unset); N = 1
PLAIN = [(3, 64, 3, 2, 1, 1, 32, 24, None), (40, 24, 3, 1, 1, 1, 7, 5, None), (32, 306, 3, 1, 6, 6, 24, 18, None),
         (136, 544, 1, 1, 0, 1, 1, 200, "0")]
HB3X3 = [(48, 48, 3, 1, 1, 1, 24, 18, "2"), (48, 96, 3, 2, 1, 1, 24, 18, "2"), (96, 40, 3, 1, 1, 1, 20, 14, "2")]
HBPW = [(136, 544, 1, 1, 0, 1, 1, 200, None), (544, 136, 1, 1, 0, 1, 1, 200, None), (64, 256, 1, 1, 0, 1, 16, 12, None),
        (40, 24, 1, 1, 0, 1, 1, 77, None)]
CASES = PLAIN + HB3X3 + HBPW
UNSUPPORTED = [(16, 16, 3, 1, -1, 1, 8, 6, None)]          # negative padding: no route takes it


def _dev():
    return torch.device("cuda", 0)


def _set_hb(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("OTPOSE_NHWC_HB", raising=False)
    else:
        monkeypatch.setenv("OTPOSE_NHWC_HB", value)


def _desc(case):
    from otpose_amd import bf16_ops as B
    cin, cout, k, stride, pad, dil, h, w, _ = case
    return B._desc(1, h, w, cin, cout, k, k, stride, pad, dil, 0)


def _nan_filled(n):
    return torch.full((n,), NAN16, dtype=torch.int16, device=_dev()).view(BF)


@pytest.mark.parametrize("dgrad", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_direct_pack_and_job_table_pack_write_the_same_bits(case, dgrad, monkeypatch):
    from otpose_amd import hip
    cin, cout, k = case[:3]
    _set_hb(monkeypatch, case[8])
    L = hip.lib()
    d = _desc(case)
    g = torch.Generator().manual_seed(sum(case[:8]) + dgrad)
    # dgrad: the (desc.Cin, desc.Cout, k, k) weight of the forward conv whose input gradient this descriptor computes
    wt = torch.randn((cin, cout, k, k) if dgrad else (cout, cin, k, k), generator=g).to(_dev())
    nbytes = L.otp_nhwc_conv_weight_bytes(ctypes.byref(d))
    assert nbytes > 0 and nbytes % 16 == 0
    direct, batched = _nan_filled(nbytes // 2), _nan_filled(nbytes // 2)
    hip.check(L.otp_nhwc_conv_pack(hip.ptr(wt), hip.ptr(direct), ctypes.byref(d), dgrad, hip.stream_of(wt)), "otp_nhwc_conv_pack")
    job = ctypes.create_string_buffer(L.otp_nhwc_conv_pack_job_bytes())
    hip.check(L.otp_nhwc_conv_pack_job(hip.ptr(wt), hip.ptr(batched), ctypes.byref(d), dgrad, job), "otp_nhwc_conv_pack_job")
    table = torch.frombuffer(bytearray(job.raw), dtype=torch.uint8).to(_dev())
    hip.check(L.otp_nhwc_conv_pack_batch(hip.ptr(table), 1, hip.stream_of(table)), "otp_nhwc_conv_pack_batch")
    torch.cuda.synchronize()
    _set_hb(monkeypatch, None)
    assert direct.numel() == batched.numel() == nbytes // 2
    assert not bool(torch.isnan(direct).any()) and not bool(torch.isnan(batched).any())
    assert torch.equal(direct.view(torch.int16), batched.view(torch.int16))
    assert int((direct != 0).sum()) == wt.numel()               # (random fp32 weights: none rounds to zero; the rest is padding)


@pytest.mark.parametrize("hb", [None, "0", "2"])
@pytest.mark.parametrize("case", CASES + UNSUPPORTED)
def test_sizes_packer_and_launch_take_the_same_descriptors(case, hb, monkeypatch):
    from otpose_amd import hip
    from otpose_amd.bf16_ops import cs
    from otpose_amd.ops import out_hw
    cin, cout, k, stride, pad, dil, h, w, _ = case
    _set_hb(monkeypatch, hb)
    L = hip.lib()
    d = _desc(case)
    g = torch.Generator().manual_seed(sum(case[:8]))
    wt = torch.randn(cout, cin, k, k, generator=g).to(_dev())
    nbytes = L.otp_nhwc_conv_weight_bytes(ctypes.byref(d))
    rows = L.otp_nhwc_conv_stats_rows(ctypes.byref(d))
    wp = torch.zeros(max(nbytes, 1 << 20) // 2, dtype=BF, device=_dev())
    rc = L.otp_nhwc_conv_pack(hip.ptr(wt), hip.ptr(wp), ctypes.byref(d), 0, hip.stream_of(wt))
    assert (nbytes != 0) == (rc == hip.OTP_OK), (nbytes, rc)
    ho, wo = out_hw(h, w, k, k, stride, pad, dil)
    x = torch.randn(1, h, w, cs(cin), generator=g).to(BF).to(_dev())
    out = torch.zeros(1, max(ho, 1), max(wo, 1), cs(cout), dtype=BF, device=_dev())
    extra = 8
    stats = torch.full((max(rows, 0) + extra, 2, cs(cout)), float("nan"), device=_dev())
    rc = L.otp_nhwc_conv_bf16(hip.ptr(x), hip.ptr(wp), None, hip.ptr(out), hip.ptr(stats), ctypes.byref(d), hip.stream_of(x))
    torch.cuda.synchronize()
    _set_hb(monkeypatch, None)
    assert (rows > 0) == (rc == hip.OTP_OK), (rows, rc)
    assert (rows > 0) == (nbytes != 0)
    assert case in UNSUPPORTED or rows > 0
    written = ~torch.isnan(stats)
    assert bool(written[:max(rows, 0)].all())                   # exactly `rows` rows are written ...
    assert not bool(written[max(rows, 0):].any())               # ... and nothing past them
