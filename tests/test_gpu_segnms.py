"""Temporal segment NMS on the GPU (csrc/segnms.hip, otpose_amd/segnms.py) against the recorded results of the reference
(tests/golden/segnms.npz): each kernel through the C ABI's Python wrapper and each drop-in name.

Kept indices, counts and classes are compared exactly; hard-NMS segments and scores too (they are copies).  Decayed scores and
voted segments are compared within a bound that was MEASURED on an MI355X: the largest relative
deviation from the file over every case here was SOFT_MEASURED for the decayed scores (device expf and a different libm,
a few ulp per round) and VOTE_MEASURED for the voted segments (the summation order); the test bound is four times that, and
stays below the 1e-4 margin every decision in the file keeps.
"""
import os

import numpy as np
import pytest
import torch

from otpose_amd import ops, segnms

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segnms.npz")
SOFT_MEASURED, VOTE_MEASURED = 2.35e-7, 1.89e-7
SOFT_BOUND, VOTE_BOUND = 4 * SOFT_MEASURED, 4 * VOTE_MEASURED
SOFT_RUNS = ((0, 0.3), (1, 0.0), (1, 0.3), (2, 0.0), (2, 0.3))
_worst = {"soft": 0.0, "vote": 0.0}


@pytest.fixture(scope="module")
def z():
    return dict(np.load(GOLDEN))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def batch(z, name):
    return dev(z[f"{name}_segs"]), dev(z[f"{name}_scores"]), dev(z[f"{name}_offsets"])


def rel_dev(got, want, kind):
    """Largest |got - want| / |want|; where the file holds 0 or NaN the result must be the same."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    exact = (want == 0) | np.isnan(want)
    assert np.array_equal(got[exact], want[exact], equal_nan=True)
    d = float((np.abs(got - want)[~exact] / np.abs(want[~exact])).max()) if (~exact).any() else 0.0
    _worst[kind] = max(_worst[kind], d)
    print(f"{kind}: largest relative deviation {d:.3e} (worst so far {_worst[kind]:.3e})")
    return d


def cut(z, tag, name, max_num, *fields):
    """The recorded uncut result cut at max_num: counts, then each field with the rows past the cut at its fill value."""
    off, counts = z[f"{name}_offsets"], z[tag + "_counts"].copy()
    out = [z[tag + "_" + f].copy() for f in fields]
    if max_num > 0:
        for g in range(len(counts)):
            counts[g] = min(counts[g], max_num)
            for a in out:
                a[off[g] + counts[g]:off[g + 1]] = -1 if a.dtype.kind == "i" else 0
    return [counts] + out


@pytest.mark.parametrize("ms, max_num", [(0.0, 0), (0.3, 0), (0.0, 1), (0.3, 5000)])
def test_hard_nms_kernel(z, ms, max_num):
    counts, keep = ops.seg_nms(*batch(z, "a"), z["thresholds"][0], ms, max_num)
    want_counts, want_keep = cut(z, f"a_hard_ms{ms}", "a", max_num, "keep")
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert np.array_equal(keep.cpu().numpy(), want_keep)


@pytest.mark.parametrize("name, method, ms, max_num", [("a", m, s, 0) for m, s in SOFT_RUNS]
                         + [("a", 2, 0.3, 1), ("a", 1, 0.0, 5000), ("b", 0, 0.0, 0)])
def test_soft_nms_kernel(z, name, method, ms, max_num):
    iou, sigma, _ = z["thresholds"]
    counts, dets, inds = ops.seg_softnms(*batch(z, name), iou, sigma, ms, method, max_num)
    want_counts, want_dets, want_inds = cut(z, f"{name}_soft_m{method}_ms{ms}", name, max_num, "dets", "inds")
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert np.array_equal(inds.cpu().numpy(), want_inds)
    dets = dets.cpu().numpy()
    assert np.array_equal(dets[:, :2], want_dets[:, :2])
    assert rel_dev(dets[:, 2], want_dets[:, 2], "soft") <= SOFT_BOUND


def _kept(z):
    """The survivors of hard NMS (min_score 0) of batch a as the voting kernel takes them."""
    off, counts, keep = z["a_offsets"], z["a_hard_ms0.0_counts"], z["a_hard_ms0.0_keep"]
    rows = np.concatenate([off[g] + keep[off[g]:off[g] + counts[g]] for g in range(len(counts))])
    return dev(z["a_segs"][rows]), dev(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))


def test_voting_kernel(z):
    nms_segs, nms_off = _kept(z)
    out = ops.seg_voting_groups(nms_segs, nms_off, *batch(z, "a"), z["thresholds"][2]).cpu().numpy()
    assert np.isnan(z["a_vote"]).any()
    assert rel_dev(out, z["a_vote"], "vote") <= VOTE_BOUND


def test_two_runs_are_bit_identical(z):
    iou, sigma, vote = z["thresholds"]
    a = batch(z, "a")
    nms_segs, nms_off = _kept(z)

    def run():
        return (*ops.seg_nms(*a, iou, 0.3, 0), *ops.seg_softnms(*a, iou, sigma, 0.0, 2, 0), *ops.seg_softnms(*a, iou, sigma, 0.3, 1, 7),
                ops.seg_voting_groups(nms_segs, nms_off, *a, vote))

    for x, y in zip(run(), run()):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_a_group_outside_the_batch_is_answered_with_zero(z):
    segs, scores, _ = batch(z, "b")
    n = segs.shape[0]
    off = torch.tensor([0, 1, n + 3, n], dtype=torch.int32, device="cuda")      # group 1 ends past the rows, group 2 runs backwards
    counts, keep = ops.seg_nms(segs, scores, off, 0.5)
    assert counts.tolist() == [1, 0, 0] and keep[0].item() == 0
    counts, _, inds = ops.seg_softnms(segs, scores, off, 0.5)
    assert counts.tolist() == [1, 0, 0] and inds[0].item() == 0


def test_the_operator_names_on_one_group(z):
    iou, sigma, vote = z["thresholds"]
    off = z["a_offsets"]
    g = 5                                                                          # 65 segments
    o0, o1 = int(off[g]), int(off[g + 1])
    segs, scores = dev(z["a_segs"][o0:o1]), dev(z["a_scores"][o0:o1])
    ident = torch.arange(o1 - o0, device="cuda")                                   # the index rides along as the class
    for max_num in (0, 3):
        s, p, c = segnms.NMSop.apply(segs, ident, scores, iou, 0.3, max_num)
        k = z["a_hard_ms0.3_counts"][g] if max_num == 0 else max_num
        want = z["a_hard_ms0.3_keep"][o0:o0 + k]
        assert np.array_equal(c.cpu().numpy(), want)
        assert torch.equal(s, segs[c]) and torch.equal(p, scores[c]) and s.is_cuda
        s, p, c = segnms.SoftNMSop.apply(segs, scores, ident, iou, sigma, 0.3, 2, max_num)
        k = z["a_soft_m2_ms0.3_counts"][g] if max_num == 0 else max_num
        assert np.array_equal(c.cpu().numpy(), z["a_soft_m2_ms0.3_inds"][o0:o0 + k])
        assert np.array_equal(s.cpu().numpy(), z["a_soft_m2_ms0.3_dets"][o0:o0 + k, :2])
        assert rel_dev(p.cpu().numpy(), z["a_soft_m2_ms0.3_dets"][o0:o0 + k, 2], "soft") <= SOFT_BOUND
    k0, k = int(z["a_hard_ms0.0_counts"][:g].sum()), int(z["a_hard_ms0.0_counts"][g])
    kept = torch.from_numpy(z["a_hard_ms0.0_keep"][o0:o0 + k]).long().cuda()
    voted = segnms.seg_voting(segs[kept], segs, scores, vote)
    assert rel_dev(voted.cpu().numpy(), z["a_vote"][k0:k0 + k], "vote") <= VOTE_BOUND


def _py_keys(z, name):
    return sorted(k[:-len("_scores")] for k in z if k.startswith(f"py_{name}_soft") and k.endswith("_scores"))


def _py_call(z, key, fn, *inputs):
    parts = key.split("_")
    iou, sigma, _ = z["thresholds"]
    return fn(*inputs, iou, float(parts[3][2:]), int(parts[5][3:]), use_soft_nms=parts[2] == "soft1",
              multiclass=parts[1] != "agn", sigma=sigma, voting_thresh=float(parts[4][4:]))


def _check_triple(z, key, out):
    s, p, c = (t.cpu().numpy() for t in out)
    assert all(t.is_cuda for t in out)
    soft, voted = "_soft1_" in key, "_vote0.75_" in key
    assert np.array_equal(c, z[key + "_cls"]) and c.dtype == z[key + "_cls"].dtype
    if soft:
        assert rel_dev(p, z[key + "_scores"], "soft") <= SOFT_BOUND
    else:
        assert np.array_equal(p, z[key + "_scores"])
    if voted:
        assert rel_dev(s, z[key + "_segs"], "vote") <= VOTE_BOUND
    else:
        assert np.array_equal(s, z[key + "_segs"])


@pytest.mark.parametrize("name", ["mc1", "mc3", "mc20", "agn"])
def test_batched_nms(z, name):
    inputs = [dev(z[f"py_{name}_in_{k}"]) for k in ("segs", "scores", "cls")]
    keys = _py_keys(z, name)
    assert len(keys) == (8 if name == "agn" else 4)
    for key in keys:
        _check_triple(z, key, _py_call(z, key, segnms.batched_nms, *inputs))


def test_three_videos_in_one_launch_equal_three_calls(z):
    names = ("mc1", "mc3", "mc20")
    videos = [tuple(dev(z[f"py_{n}_in_{k}"]) for k in ("segs", "scores", "cls")) for n in names]
    empty = (videos[0][0][:0], videos[0][1][:0], videos[0][2][:0])
    for k1, k3, k20 in zip(*(_py_keys(z, n) for n in names)):
        assert k1.split("_")[2:] == k3.split("_")[2:] == k20.split("_")[2:]
        together = _py_call(z, k1, segnms.batched_nms_videos, videos[:2] + [empty] + videos[2:])
        assert len(together) == 4 and together[2][0].shape == (0, 2)
        for key, video, got in zip((k1, k3, k20), videos, together[:2] + together[3:]):
            alone = _py_call(z, key, segnms.batched_nms, *video)
            assert all(torch.equal(a, b) for a, b in zip(alone, got))
            _check_triple(z, key, got)
    agn = [dev(z[f"py_agn_in_{k}"]) for k in ("segs", "scores", "cls")]            # class-agnostic: a group is a video
    for key in _py_keys(z, "agn"):
        together = _py_call(z, key, segnms.batched_nms_videos, [tuple(agn), videos[1]])
        _check_triple(z, key, together[0])
        alone = _py_call(z, key, segnms.batched_nms, *videos[1])
        assert all(torch.equal(a, b) for a, b in zip(alone, together[1]))


def test_the_bounds_stay_below_the_decision_margin():
    assert 0 < SOFT_BOUND < 1e-4 and 0 < VOTE_BOUND < 1e-4
