"""csrc/pointx.hip, pointx_pair_kernel: a layer1 Bottleneck's conv3 (+ residual, ReLU) and the next Bottleneck's conv1 (ReLU, S8
records) as one launch (model/HRNet.py:551-571).  The launch keeps the product order of the two kernels it replaces, so its two
outputs are compared bit for bit with otp_pointwise_x3 followed by otp_pointwise_x3_s8, and with fp64 at the 2e-5 of the output
range that test_pointwise_x3_matches_fp64 uses.  A workgroup tile is 128 tokens, a wave owns 32, a lane a pixel pair."""
import pytest
import torch

from otpose_amd import OTPose, cfg1, hip, ops, tiny_cfg
from otpose_amd import synthetic as S
from tests.conftest import seeded

pytestmark = pytest.mark.gpu
CMID, COUT2 = 256, 64
# (B, Cin, residual, (H, W)): T = H * W
CASES = [(3, 64, True, (13, 10)),      # T = 130: one full tile plus a 2-token ragged tile
         (2, 64, True, (12, 8)),       # T = 96: less than one tile, one wave idle
         (2, 128, False, (43, 6)),     # T = 258: input a channel slice of a wider buffer; the residual-free instantiation
         (1, 64, True, (96, 72))]      # T = 6912: one real frame, all tiles of a map
_cache = {}


def _close(a, b, tol=2e-5):
    a = a.detach().cpu()
    assert a.shape == b.shape
    err = float((a - b).abs().max())
    print(f"max abs err {err:.3e} of range {float(b.abs().max()):.3f}")
    assert err <= tol * max(1.0, float(b.abs().max())), f"max abs err {err} (ref max {float(b.abs().max())})"


def _case(case):
    """Inputs, the pair launch's two outputs and the two-launch outputs of one case (computed once, shared, left unchanged)."""
    if case in _cache:
        return _cache[case]
    B, cin, res, (h, w) = case
    xoff = 16 if cin == 128 else 0
    xt = seeded((B, cin + 2 * xoff, h, w), 171)                        # Cin = 128: channels [16, 144) of a 160-channel buffer
    w1, sc1, sh1 = seeded((CMID, cin), 172) / cin ** 0.5, 1.0 + 0.3 * seeded((CMID,), 173), seeded((CMID,), 174)
    w2, sc2, sh2 = seeded((COUT2, CMID), 175) / CMID ** 0.5, 1.0 + 0.3 * seeded((COUT2,), 176), seeded((COUT2,), 177)
    rt = seeded((B, CMID + 8, h, w), 178) if res else None              # residual: channels [8, 264)
    c = lambda t: t.cuda()                                              # noqa: E731
    xv = ops.View(c(xt), xoff, cin)
    rv = ops.View(c(rt), 8, CMID) if res else None
    assert ops.pointwise_x3_pair_supported(cin, CMID, COUT2, h * w)
    # today's two launches
    o_ref = torch.full((B, CMID + 5, h, w), 7.0, device="cuda")         # output: channels [2, 258)
    ops.pointwise_x3(xv, ops.pack_pointwise_x3(c(w1), c(sc1), c(sh1)), ops.View(o_ref, 2, CMID), rv, True)
    s8_ref = ops.pointwise_x3_s8(ops.View(o_ref, 2, CMID), ops.pack_pointwise_x3_s8(c(w2), c(sc2), c(sh2)), COUT2, relu=True)
    # the pair launch
    o = torch.full((B, CMID + 5, h, w), 7.0, device="cuda")
    s8 = ops.pointwise_x3_pair(xv, ops.pack_pointwise_x3_pair(c(w1), c(sc1), c(sh1), c(w2), c(sc2), c(sh2)),
                               ops.View(o, 2, CMID), COUT2, res=rv)
    torch.cuda.synchronize()
    _cache[case] = dict(x=xt[:, xoff:xoff + cin], r=rt[:, 8:8 + CMID] if res else None, w1=w1, sc1=sc1, sh1=sh1, w2=w2, sc2=sc2,
                        sh2=sh2, o=o, s8=s8, o_ref=o_ref, s8_ref=s8_ref)
    return _cache[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[0]}-cin{c[1]}-T{c[3][0] * c[3][1]}")
def test_pair_launch_is_bit_identical_to_the_two_launches(case):
    d = _case(case)
    assert torch.equal(d["o"], d["o_ref"])            # the fp32 NCHW tensor, the untouched channels around the slice included
    assert bool((d["o"][:, :2] == 7).all()) and bool((d["o"][:, 2 + CMID:] == 7).all())
    assert torch.equal(d["s8"], d["s8_ref"])          # the S8 image of the next block's conv1


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[0]}-cin{c[1]}-T{c[3][0] * c[3][1]}")
def test_pair_launch_matches_fp64(case):
    d = _case(case)
    B, _, _, (h, w) = case
    bc = lambda v: v.double()[None, :, None, None]                      # noqa: E731
    y = torch.einsum("oc,bchw->bohw", d["w1"].double(), d["x"].double()) * bc(d["sc1"]) + bc(d["sh1"])
    if d["r"] is not None:
        y = y + d["r"].double()
    y = y.clamp_min(0)
    z = (torch.einsum("oc,bchw->bohw", d["w2"].double(), y) * bc(d["sc2"]) + bc(d["sh2"])).clamp_min(0)
    _close(d["o"][:, 2:2 + CMID], y.float(), 2e-5)
    _close(ops.s8_unpack(d["s8"], B, COUT2, h, w), z.float(), 2e-5)


def test_unsupported_shapes_are_refused():
    assert not ops.pointwise_x3_pair_supported(256, CMID, COUT2, 96) and not ops.pointwise_x3_pair_supported(64, 128, COUT2, 96)
    assert not ops.pointwise_x3_pair_supported(64, CMID, 32, 96) and not ops.pointwise_x3_pair_supported(64, CMID, COUT2, 97)
    L = hip.lib()
    assert L.otp_pointwise_x3_pair_weight_bytes(64, CMID, COUT2) == (64 + 2 + 64 + 2) * 1024
    assert L.otp_pointwise_x3_pair_weight_bytes(128, CMID, COUT2) == (128 + 2 + 64 + 2) * 1024
    assert L.otp_pointwise_x3_pair(None, None, None, None, None, 1, 64, CMID, COUT2, 96, 64, 0, 256, 0, 256, 0, 1, 1, None) == -1


@pytest.mark.range_overflow_expected
def test_range_guard_covers_the_conv3_result():
    """conv3 results past 65504 set the sticky word (family 4, pointx) before the clamp; the same launch in range leaves it clear."""
    B, cin, h, w = 1, 64, 12, 8
    w1, w2 = seeded((CMID, cin), 181) / cin ** 0.5, seeded((COUT2, CMID), 182) / CMID ** 0.5
    pk = ops.pack_pointwise_x3_pair(w1.cuda(), None, None, w2.cuda(), None, None)
    x = seeded((B, cin, h, w), 183).cuda()
    r = torch.zeros(B, CMID, h, w, device="cuda")
    o = torch.empty(B, CMID, h, w, device="cuda")
    torch.cuda.synchronize()
    hip.lib().otp_range_flag_read(1)
    ops.pointwise_x3_pair(ops.View(x), pk, ops.View(o), COUT2, res=ops.View(r))
    torch.cuda.synchronize()
    assert hip.lib().otp_range_flag_read(1) == 0
    r[0, 37, 5, 3] = 7.0e4                                              # one residual value carries one result past the limit
    ops.pointwise_x3_pair(ops.View(x), pk, ops.View(o), COUT2, res=ops.View(r))
    torch.cuda.synchronize()
    assert hip.lib().otp_range_flag_read(1) == 4


def _forward(cfg, batch, pair):
    import os
    os.environ["OTPOSE_L1_PAIR"] = pair
    try:
        m = OTPose(cfg)
        S.fill_synthetic_(m)
        m = m.cuda().eval()
        x, margin = S.synthetic_clip(batch, cfg.MODEL.IMAGE_SIZE)
        with torch.no_grad():
            outs = m(x.cuda(), margin=margin.cuda())
        torch.cuda.synchronize()
        return [o_.cpu().clone() for o_ in outs], m._engine.l1_pairs
    finally:
        del os.environ["OTPOSE_L1_PAIR"]


@pytest.mark.parametrize("name", ["tiny", "cfg1"])
def test_engine_outputs_are_bit_identical_with_the_pair_switch_on_and_off(name):
    """OTPOSE_L1_PAIR=1 (default) against =0 (the two launches): the arithmetic and its order are unchanged, so all seven outputs
    are equal bit for bit."""
    cfg, batch = (tiny_cfg(8, (64, 96)), 2) if name == "tiny" else (cfg1(), 1)
    on, n_on = _forward(cfg, batch, "1")
    off, n_off = _forward(cfg, batch, "0")
    assert n_on == 3 and n_off == 0                   # layer1's three block boundaries (HRNet.py:240-247: four Bottlenecks)
    assert len(on) == len(off) == 7
    for a, b in zip(on, off):
        assert torch.equal(a, b)
