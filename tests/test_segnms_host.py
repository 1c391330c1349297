"""Temporal segment NMS without a GPU: the restatement tests/segnms_ref.py against the recorded results of the reference
(tests/golden/segnms.npz, written by tests/golden/make_golden_segnms.py), the drop-in names' signatures, what they answer
to CPU tensors and to an empty input, and the C entry points' argument checks."""
import inspect
import os

import numpy as np
import pytest
import torch

from otpose_amd import hip, ops, segnms
from tests import segnms_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segnms.npz")
HARD_RUNS = (0.0, 0.3)
SOFT_RUNS = ((0, 0.3), (1, 0.0), (1, 0.3), (2, 0.0), (2, 0.3))
PY_RUNS = ((True, 0.001), (True, 0.3), (False, 0.0), (False, 0.3))
# The generator asserts the restatement equal to the built extension bit for bit.  Here the decayed scores and voted segments
# are allowed 1e-5 relative: the C library's expf may differ in the last place between the machine that wrote the file and the
# one that reads it (a few 6e-8 steps over the rounds of one segment), and the file's voted segments are torch's matrix product,
# whose summation order is not numpy's.  1e-5 is a tenth of the 1e-4 margin every decision in the file keeps, so indices,
# counts and classes are compared exactly.
RTOL = 1e-5


@pytest.fixture(scope="module")
def z():
    return dict(np.load(GOLDEN))


def _groups(z, name):
    off = z[f"{name}_offsets"]
    for g in range(len(off) - 1):
        yield g, int(off[g]), int(off[g + 1])


@pytest.mark.parametrize("name, soft_runs", [("a", SOFT_RUNS), ("b", ((0, 0.0),))])
def test_restatement_reproduces_the_recorded_kernel_cases(z, name, soft_runs):
    iou, sigma, vote = z["thresholds"]
    segs, scores = z[f"{name}_segs"], z[f"{name}_scores"]
    sizes = []
    for g, o0, o1 in _groups(z, name):
        s, p = segs[o0:o1], scores[o0:o1]
        sizes.append(o1 - o0)
        for ms in HARD_RUNS:
            idx = R.NMSop_apply(s, np.arange(o1 - o0), p, iou, ms, 0)[2]
            assert len(idx) == z[f"{name}_hard_ms{ms}_counts"][g]
            assert np.array_equal(idx, z[f"{name}_hard_ms{ms}_keep"][o0:o0 + len(idx)])
            assert (z[f"{name}_hard_ms{ms}_keep"][o0 + len(idx):o1] == -1).all()
        for method, ms in soft_runs:
            tag = f"{name}_soft_m{method}_ms{ms}"
            dets, inds = R.softnms_1d(s, p, iou, sigma, ms, method)
            assert len(inds) == z[tag + "_counts"][g]
            assert np.array_equal(inds, z[tag + "_inds"][o0:o0 + len(inds)])
            np.testing.assert_array_equal(dets[:len(inds), :2], z[tag + "_dets"][o0:o0 + len(inds), :2])
            np.testing.assert_allclose(dets[:len(inds), 2], z[tag + "_dets"][o0:o0 + len(inds), 2], rtol=RTOL, atol=0)
    if name == "a":
        assert sizes[:8] == [0, 1, 2, 63, 64, 65, 200, 1025]
        assert 1025 > hip.CONSTANTS["OTP_SEG_NMS_LDS_CAP"] >= 200          # the file reaches both the LDS and the workspace path
        counts = z["a_hard_ms0.0_counts"]
        assert counts[8] == 1 and counts[9] == sizes[9]                     # identical: one survives; disjoint: all do
        k0 = 0
        for g, o0, o1 in _groups(z, "a"):
            kept = z["a_hard_ms0.0_keep"][o0:o0 + counts[g]]
            mine = R.seg_voting(segs[o0:o1][kept], segs[o0:o1], scores[o0:o1], vote)
            want = z["a_vote"][k0:k0 + counts[g]]
            assert np.array_equal(np.isnan(mine), np.isnan(want))
            np.testing.assert_allclose(mine, want, rtol=RTOL, atol=0, equal_nan=True)
            k0 += counts[g]
        assert np.isnan(z["a_vote"]).any()                                  # a kept zero-length segment: 0 / 0, as in the reference


def _py_keys(z, name):
    return sorted(k[:-len("_scores")] for k in z if k.startswith(f"py_{name}_soft") and k.endswith("_scores"))


def _py_args(key):
    parts = key.split("_")
    return dict(soft=parts[2] == "soft1", ms=float(parts[3][2:]), vote=float(parts[4][4:]), max_seg=int(parts[5][3:]),
                multiclass=parts[1] != "agn")


@pytest.mark.parametrize("name", ["mc1", "mc3", "mc20", "agn"])
def test_restatement_reproduces_the_recorded_batched_nms(z, name):
    iou, sigma, _ = z["thresholds"]
    segs, scores, cls = (z[f"py_{name}_in_{k}"] for k in ("segs", "scores", "cls"))
    keys = _py_keys(z, name)
    assert len(keys) == (8 if name == "agn" else 4)
    for key in keys:
        a = _py_args(key)
        s, p, c = R.batched_nms(segs, scores, cls, iou, a["ms"], a["max_seg"], use_soft_nms=a["soft"],
                                multiclass=a["multiclass"], sigma=sigma, voting_thresh=a["vote"])
        assert np.array_equal(c, z[key + "_cls"]) and c.dtype == z[key + "_cls"].dtype
        np.testing.assert_allclose(p, z[key + "_scores"], rtol=RTOL, atol=0)
        np.testing.assert_allclose(s, z[key + "_segs"], rtol=RTOL, atol=0)
        assert len(p) <= a["max_seg"]


def test_drop_in_names_keep_the_reference_signatures():
    def names(f):
        return list(inspect.signature(f).parameters)

    assert names(segnms.NMSop.forward) == ["ctx", "segs", "cls_idxs", "scores", "iou_threshold", "min_score", "max_num"]
    assert names(segnms.SoftNMSop.forward) == ["ctx", "segs", "scores", "cls_idxs", "iou_threshold", "sigma", "min_score",
                                               "method", "max_num"]
    assert names(segnms.seg_voting) == ["nms_segs", "all_segs", "all_scores", "iou_threshold", "score_offset"]
    assert inspect.signature(segnms.seg_voting).parameters["score_offset"].default == 1.5
    sig = inspect.signature(segnms.batched_nms)
    assert list(sig.parameters) == ["segs", "scores", "cls_idxs", "iou_threshold", "min_score", "max_seg_num", "use_soft_nms",
                                    "multiclass", "sigma", "voting_thresh"]
    assert [sig.parameters[k].default for k in ("use_soft_nms", "multiclass", "sigma", "voting_thresh")] == [True, True, 0.5, 0.75]
    assert list(inspect.signature(segnms.batched_nms_videos).parameters)[1:] == list(sig.parameters)[3:]
    assert issubclass(segnms.NMSop, torch.autograd.Function) and issubclass(segnms.SoftNMSop, torch.autograd.Function)


def test_cpu_tensors_raise():
    segs, scores, cls = torch.tensor([[0.0, 1.0], [0.5, 2.0]]), torch.tensor([0.9, 0.8]), torch.tensor([0, 0])
    off = torch.tensor([0, 2], dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        segnms.NMSop.apply(segs, cls, scores, 0.5, 0.0, 0)
    with pytest.raises(NotImplementedError):
        segnms.SoftNMSop.apply(segs, scores, cls, 0.5, 0.5, 0.0, 2, 0)
    with pytest.raises(NotImplementedError):
        segnms.seg_voting(segs, segs, scores, 0.75)
    with pytest.raises(NotImplementedError):
        segnms.batched_nms(segs, scores, cls, 0.5, 0.0, 10)
    with pytest.raises(NotImplementedError):
        segnms.batched_nms_videos([(segs, scores, cls)], 0.5, 0.0, 10)
    for fn in (ops.seg_nms, ops.seg_softnms):
        with pytest.raises(NotImplementedError):
            fn(segs, scores, off, 0.5)
    with pytest.raises(NotImplementedError):
        ops.seg_voting_groups(segs, off, segs, scores, off, 0.75)


@pytest.mark.parametrize("cls_dtype", [torch.int64, torch.int32])
def test_empty_input_returns_the_reference_triple(cls_dtype):
    """nms.py:119-122: (0, 2) float32, (0,) float32, (0,) of the class tensor's dtype - no kernel runs, so no GPU is needed."""
    e = (torch.zeros(0, 2), torch.zeros(0), torch.zeros(0, dtype=cls_dtype))
    for out in (segnms.batched_nms(*e, 0.5, 0.001, 100), segnms.batched_nms_videos([e, e], 0.5, 0.001, 100)[1]):
        assert [tuple(t.shape) for t in out] == [(0, 2), (0,), (0,)]
        assert [t.dtype for t in out] == [torch.float32, torch.float32, cls_dtype]
    assert segnms.batched_nms_videos([], 0.5, 0.001, 100) == []
    assert [tuple(t.shape) for t in segnms.NMSop.apply(e[0], e[2], e[1], 0.5, 0.0, 0)] == [(0, 2), (0,), (0,)]
    assert [tuple(t.shape) for t in segnms.SoftNMSop.apply(*e, 0.5, 0.5, 0.0, 2, 0)] == [(0, 2), (0,), (0,)]


def test_header_exports_and_argument_checks():
    L = hip.lib()
    for name in ("otp_seg_nms", "otp_seg_softnms", "otp_seg_voting", "otp_seg_nms_workspace"):
        assert name in hip.SIGNATURES and hasattr(L, name)
    words = hip.CONSTANTS["OTP_SEG_NMS_WS_WORDS"]
    assert L.otp_seg_nms_workspace(3, 1000) == words * 1000 * 4 == L.otp_seg_nms_workspace(1, 1000)
    assert L.otp_seg_nms_workspace(0, 10) == 0 and L.otp_seg_nms_workspace(2, 0) == 0
    p = 64                                                                   # any non-null address: every call below returns first
    bad, short = hip.CONSTANTS["OTP_ERR_BAD_ARG"], hip.CONSTANTS["OTP_ERR_WORKSPACE"]
    assert L.otp_seg_nms(None, p, p, 1, 4, 0.5, 0.0, 0, p, 1 << 20, p, p, None) == bad
    assert L.otp_seg_nms(p, p, p, 0, 4, 0.5, 0.0, 0, p, 1 << 20, p, p, None) == bad
    assert L.otp_seg_nms(p, p, p, 1, 4, float("nan"), 0.0, 0, p, 1 << 20, p, p, None) == bad
    assert L.otp_seg_nms(p, p, p, 1, 4, 0.5, 0.0, 0, p, words * 4 * 4 - 1, p, p, None) == short
    assert L.otp_seg_softnms(p, p, p, 1, 4, 0.5, 0.5, 0.0, 3, 0, p, 1 << 20, p, p, p, None) == bad
    assert L.otp_seg_softnms(p, p, p, 1, 4, 0.5, 0.0, 0.0, 2, 0, p, 1 << 20, p, p, p, None) == bad      # gaussian needs sigma > 0
    assert L.otp_seg_softnms(p, p, p, 1, 4, 0.5, 0.5, 0.0, 2, 0, p, 8, p, p, p, None) == short
    assert L.otp_seg_voting(p, p, p, p, p, 1, 0, 4, 0.75, p, None) == bad
    assert L.otp_seg_voting(p, None, p, p, p, 1, 2, 4, 0.75, p, None) == bad
    assert L.otp_seg_nms(p, p, p, 1, 1 << 28, 0.5, 0.0, 0, p, 1 << 40, p, p, None) == hip.CONSTANTS["OTP_ERR_UNSUPPORTED"]
