"""Pose NMS on the GPU: ``ops.pose_nms`` against the numpy restatement (tests/pose_nms_ref.py) on a seeded case of 300
frames, and ``PoseTrackEvaluator(nms=...)`` end to end.  ``keep``, ``rank`` and the person scores are compared exactly, the
OKS rows within 1e-12 absolute and the soft scores within 1e-12 relative: what can differ is ``exp`` (device libm and numpy
are each within about 1 ulp; 17 terms <= 1 give under 4e-15; the linear soft type's ``1 - oks`` magnifies that next to
oks = 1 - seen on the MI355X: 3.3e-16 on the OKS, 6.5e-13 relative on linear soft scores).  Every frame and person is compared; the input conditions (a)
and (b) of ``pose_nms_ref.input_conditions`` are asserted on the restatement's own values and exclude nothing."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from otpose_amd import hip, ops, posetrack_eval as PE, synthetic as S
from tests import pose_nms_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posetrack_ap.npz")
IN_VIS = 0.2
HARD = [dict(oks_thresh=t, oks_in_vis_thre=v) for t in (0.5, 0.9) for v in (None, 0.3)]
SOFT = [dict(oks_thresh=t, soft=True, soft_type=k) for t in (0.5, 0.9) for k in ("gaussian", "linear")]


def _id(s):
    return "-".join(f"{v}" for v in s.values())


@pytest.fixture(scope="module")
def case():
    frames, preds, box, fid, area, special = S.pose_nms_case(300, 0)
    g = PE.pack_ground_truth(frames)
    pr_off, pr_sample = PE.pack_predictions(g["frame_map"], fid, len(g["kept"]))
    host = [pr_off, pr_sample, np.ascontiguousarray(preds[:, :, :2]), np.ascontiguousarray(preds[:, :, 2:]), box, area]
    # what the case must hold
    n = np.diff(pr_off)
    assert {1, 2, 3, 63, 64} <= set(n.tolist()) and n.max() == ops.POSEVAL_MAX_PR
    assert (pr_sample < 0).any() and (n[pr_sample[pr_off[:-1]] < 0] == 1).all()          # frames with the placeholder only
    where = {k: int(np.nonzero(pr_sample == s)[0][0]) for k, s in special.items()}        # all in evaluated frames
    frame_of = np.repeat(np.arange(n.size), n)
    named = ("exact", "low_vis", "zero_area", "equal", "nan_xy", "nan_score")
    assert len({frame_of[where[k]] for k in named}) == len(named)
    for k in ("exact", "zero_area", "equal"):
        assert frame_of[where[k]] == frame_of[where[k + "_of"]]
    keep, score, rank, oks = R.pose_nms_ref(*host, oks_thresh=0.9, in_vis_thre=IN_VIS, return_oks=True)
    local = lambda k: where[k] - pr_off[frame_of[where[k]]]
    assert oks[where["exact_of"], local("exact")] == 1.0 and oks[where["zero_area_of"], local("zero_area")] == 1.0
    assert score[where["low_vis"]] == 0.0 and (preds[special["low_vis"], :, 2] < IN_VIS).all()
    assert area[special["zero_area"]] == 0.0
    assert score[where["equal"]].tobytes() == score[where["equal_of"]].tobytes() and score[where["equal"]] > 0
    assert np.isnan(oks[where["nan_xy"], :n[frame_of[where["nan_xy"]]]]).all() and np.isnan(score[where["nan_score"]])
    assert np.isnan(score).sum() == 1 and np.isnan(preds[:, :, :2]).any(2).any(1).sum() == 1
    # jittered duplicates between 0.5 and 20 px are what fills the high end of the tile
    assert ((oks > 0.5) & (oks < 1.0)).sum() > 500
    dev = [torch.from_numpy(a).cuda() for a in host]
    return {"frames": frames, "gt": g, "preds": preds, "box": box, "fid": fid, "area": area, "host": host, "dev": dev,
            "pr_off": pr_off, "pr_sample": pr_sample, "where": where, "frame_of": frame_of}


def _compare(case, settings):
    want_keep, want_score, want_rank, want_oks = R.input_conditions(*case["host"], in_vis_thre=IN_VIS, **settings)
    keep, score, rank, oks = ops.pose_nms(*case["dev"], in_vis_thre=IN_VIS, return_oks=True, **settings)
    assert keep.dtype == torch.bool and score.dtype == torch.float64 and rank.dtype == torch.int32
    assert oks.shape == (want_keep.size, 64) and oks.dtype == torch.float64
    oks, score = oks.cpu().numpy(), score.cpu().numpy()
    assert np.array_equal(np.isnan(oks), np.isnan(want_oks))
    diff = np.abs(oks - want_oks)[~np.isnan(want_oks)].max()
    print("largest OKS difference", diff)
    assert diff <= 1e-12
    assert np.array_equal(keep.cpu().numpy(), want_keep)
    assert np.array_equal(rank.cpu().numpy(), want_rank)
    return score, want_score


@pytest.mark.parametrize("settings", HARD, ids=_id)
def test_hard_nms_matches_the_restatement(case, settings):
    score, want = _compare(case, settings)
    assert np.array_equal(score.view(np.int64), want.view(np.int64))                     # bit for bit
    keep2 = ops.pose_nms(*case["dev"], in_vis_thre=IN_VIS, **settings)[0]              # without the OKS output
    assert torch.equal(keep2, ops.pose_nms(*case["dev"], in_vis_thre=IN_VIS, return_oks=True, **settings)[0])


@pytest.mark.parametrize("settings", SOFT, ids=_id)
def test_soft_nms_matches_the_restatement(case, settings):
    score, want = _compare(case, settings)
    assert np.array_equal(np.isnan(score), np.isnan(want))
    m = ~np.isnan(want)
    rel = np.abs(score[m] - want[m]) / np.where(want[m] != 0, np.abs(want[m]), 1.0)
    print("largest relative soft-score difference", rel.max())
    assert rel.max() <= 1e-12
    n = np.diff(case["pr_off"])
    keep = ops.pose_nms(*case["dev"], in_vis_thre=IN_VIS, **settings)[0].cpu().numpy()
    assert np.array_equal(np.add.reduceat(keep.astype(np.int64), case["pr_off"][:-1]), np.minimum(n, 20))


def test_threshold_one_keeps_every_person_with_finite_coordinates(case):
    # no condition (a) here: an OKS is a sum of 17 terms <= 1 divided by 17, so it cannot exceed 1 in either libm
    keep = ops.pose_nms(*case["dev"], oks_thresh=1.0, in_vis_thre=IN_VIS)[0].cpu().numpy()
    want = R.pose_nms_ref(*case["host"], oks_thresh=1.0, in_vis_thre=IN_VIS)[0]
    assert np.array_equal(keep, want)
    nan_xy = case["where"]["nan_xy"]
    assert not keep[nan_xy] and keep[np.arange(keep.size) != nan_xy].all()
    # the NaN person in front of its frame (box score 50) is kept and removes the rest of the frame
    box = case["box"].copy()
    box[case["pr_sample"][nan_xy]] = 50.0
    keep = ops.pose_nms(*case["dev"][:4], torch.from_numpy(box).cuda(), case["dev"][5], oks_thresh=1.0,
                        in_vis_thre=IN_VIS)[0].cpu().numpy()
    same = case["frame_of"] == case["frame_of"][nan_xy]
    assert keep[nan_xy] and keep[same].sum() == 1 and keep[~same].all()


def test_arguments_are_checked_on_the_host(case):
    dev = case["dev"]
    n = ops.POSEVAL_MAX_PR + 1
    f = case["pr_off"].size - 1
    over = list(dev)
    over[0] = torch.tensor([0, n] + [n] * (f - 1), dtype=torch.int32).cuda()
    over[1] = torch.zeros(n, dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match="limit"):
        ops.pose_nms(*over, oks_thresh=0.9)
    bad = list(dev)
    bad[0] = dev[0].clone()
    bad[0][-1] += 1
    with pytest.raises(ValueError, match="offsets"):
        ops.pose_nms(*bad, oks_thresh=0.9)
    bad = list(dev)
    bad[1] = torch.where(dev[1] >= 0, dev[1] + case["preds"].shape[0], dev[1])
    with pytest.raises(ValueError, match="pr_sample"):
        ops.pose_nms(*bad, oks_thresh=0.9)
    for kw in (dict(oks_thresh=0.0), dict(oks_thresh=math.inf), dict(oks_thresh=math.nan), dict(oks_thresh=0.9, max_dets=0),
               dict(oks_thresh=0.9, sigmas=R.COCO_SIGMAS[:16]), dict(oks_thresh=0.9, sigmas=[0.0] * 17),
               dict(oks_thresh=0.9, sigmas=[math.inf] * 17), dict(oks_thresh=0.9, soft=True, soft_type="exp")):
        with pytest.raises(ValueError):
            ops.pose_nms(*dev, **kw)
    with pytest.raises(NotImplementedError):
        ops.pose_nms(*[torch.from_numpy(a) for a in case["host"]], oks_thresh=0.9)
    with pytest.raises(TypeError):
        ops.pose_nms(*dev[:5], dev[5].float(), oks_thresh=0.9)


@pytest.mark.parametrize("settings", [HARD[2], SOFT[0]], ids=_id)
def test_evaluator_with_nms_equals_evaluator_fed_the_survivors(case, settings):
    want_keep = R.input_conditions(*case["host"], in_vis_thre=IN_VIS, **settings)[0]
    survivors = np.sort(case["pr_sample"][want_keep & (case["pr_sample"] >= 0)]).astype(np.int64)
    assert 0 < survivors.size < (case["pr_sample"] >= 0).sum()
    p = torch.from_numpy(case["preds"]).cuda()
    xy, mv = p[:, :, :2].contiguous(), p[:, :, 2:].contiguous()
    nms = PE.PoseNMS(in_vis_thre=IN_VIS, **settings)
    ev = PE.PoseTrackEvaluator(case["gt"], nms=nms)
    cut = case["fid"].size // 3                                       # two ragged adds, one by area and one by scale
    ev.add(xy[:cut], mv[:cut], case["box"][:cut], case["fid"][:cut], area=case["area"][:cut])
    ev.add(xy[cut:], mv[cut:], case["box"][cut:], case["fid"][cut:], area=torch.from_numpy(case["area"][cut:]))
    assert np.array_equal(ev.kept_samples(), survivors)
    idx = torch.from_numpy(survivors).cuda()
    plain = PE.PoseTrackEvaluator(case["gt"])
    plain.add(xy[idx], mv[idx], case["box"][survivors], case["fid"][survivors])
    got, want = ev.assign(), plain.assign()
    for a, b in zip(got[:3], want[:3]):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))
    assert np.array_equal(got[3], want[3])                            # the compacted offsets
    assert np.array_equal(np.where(want[4] >= 0, survivors[np.maximum(want[4], 0)], -1), got[4])
    a, b = ev.summarize(), plain.summarize()
    for k in ("ap", "precision", "recall"):
        assert a[k].tobytes() == b[k].tobytes()
    assert np.array(list(a["table"].values())).tobytes() == np.array(list(b["table"].values())).tobytes()
    rects = sum(len(fr["annorect"]) for fr in ev.annolist())
    dropped = case["gt"]["frame_map"][case["fid"]] < 0
    empty = case["gt"]["num_frames"] - np.unique(case["fid"]).size
    assert rects == survivors.size + dropped.sum() + empty


def test_scale_gives_the_area_of_the_crop(case):
    rng = np.random.default_rng(5)
    scale = rng.uniform(0.3, 2.0, (case["fid"].size, 2)).astype(np.float32)
    p = torch.from_numpy(case["preds"]).cuda()
    by = {}
    for key, kw in (("scale", {"scale": torch.from_numpy(scale).cuda()}),
                    ("area", {"area": (scale.astype(np.float64) * 200.0).prod(1)})):
        ev = PE.PoseTrackEvaluator(case["gt"], nms=PE.PoseNMS(oks_thresh=0.9, in_vis_thre=IN_VIS))
        ev.add(p[:, :, :2].contiguous(), p[:, :, 2:].contiguous(), case["box"], case["fid"], **kw)
        by[key] = ev.kept_samples()
    assert np.array_equal(by["scale"], by["area"])


def test_without_nms_the_evaluator_is_the_parent_commits():
    z = np.load(GOLDEN)
    gold = {k: z[k] for k in z.files}
    frames = S.posetrack_eval_case(int(gold["frames"]), int(gold["seed"]))[0]
    ev = PE.PoseTrackEvaluator(frames, nms=None)
    p = torch.from_numpy(gold["preds"]).cuda()
    ev.add(p[:, :, :2], p[:, :, 2:], gold["box_score"], gold["frame_id"])
    labels, scores, ngt, pr_off, pr_sample = ev.assign()
    assert np.array_equal(labels.cpu().numpy(), gold["labels"])
    assert np.array_equal(scores.cpu().numpy().view(np.int64), gold["scores"].view(np.int64))
    assert np.array_equal(ngt.cpu().numpy(), gold["nGTall"])
    assert np.array_equal(pr_off, gold["pr_off"]) and np.array_equal(pr_sample, gold["pr_sample"])
    res = ev.summarize()
    for k, want in (("ap", gold["apAll"]), ("precision", gold["preAll"]), ("recall", gold["recAll"])):
        assert np.abs(res[k] - want).max() <= 1e-9
    assert np.array_equal(ev.kept_samples(), np.sort(gold["pr_sample"][gold["pr_sample"] >= 0]))
    assert PE.PoseTrackEvaluator(frames).nms is None


def test_one_launch_is_graph_capturable(case):
    dev = case["dev"]
    npr, f, n = dev[1].numel(), dev[0].numel() - 1, dev[2].shape[0]
    eager = ops.pose_nms(*dev, oks_thresh=0.9, in_vis_thre=IN_VIS)
    keep = torch.zeros(npr, dtype=torch.int8, device="cuda")
    score = torch.zeros(npr, dtype=torch.float64, device="cuda")
    rank = torch.zeros(npr, dtype=torch.int32, device="cuda")
    sig = (ctypes.c_double * 17)(*ops.COCO_SIGMAS)
    L, P = hip.lib(), hip.ptr

    def launch():
        hip.check(L.otp_pose_nms(*[P(a) for a in dev], sig, IN_VIS, 0.9, math.nan, 0, 20, P(keep), P(score), P(rank), None,
                                 f, npr, n, hip.stream_of(keep)), "otp_pose_nms")

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    keep.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(keep.view(torch.bool), eager[0]) and torch.equal(rank, eager[2])
    assert torch.equal(score.view(torch.int64), eager[1].view(torch.int64))
