"""Host side of the pose NMS: the numpy restatement (tests/pose_nms_ref.py) against the loop-by-loop transcription of the
HRNet functions it follows, the order rules on hand-made frames, the C entry point's argument check, ``PoseNMS.from_cfg``
and the evaluator's ``add``.  No GPU needed."""
import ctypes
import math

import numpy as np
import pytest
import torch

from otpose_amd import hip, posetrack_eval as PE, synthetic as S
from otpose_amd.config import CfgNode
from tests import pose_nms_ref as R

IN_VIS = 0.2


@pytest.fixture(scope="module")
def case():
    frames, preds, box, fid, area, special = S.pose_nms_case(40, 4)
    g = PE.pack_ground_truth(frames)
    pr_off, pr_sample = PE.pack_predictions(g["frame_map"], fid, len(g["kept"]))
    return pr_off, pr_sample, preds, box, area


def _frames(case):
    """Per frame with a real person: (slice of the packed persons, HRNet's kpts_db before rescoring)."""
    pr_off, pr_sample, preds, box, area = case
    for a, b in zip(pr_off[:-1], pr_off[1:]):
        if pr_sample[a] < 0:
            continue
        db = [{"keypoints": preds[s].astype(np.float64), "score": float(box[s]), "area": float(area[s])}
              for s in pr_sample[a:b]]
        R.hrnet_rescore_persons(db, IN_VIS)
        yield a, b, db


def _args(case):
    pr_off, pr_sample, preds, box, area = case
    return pr_off, pr_sample, preds[:, :, :2], preds[:, :, 2], box, area


@pytest.mark.parametrize("oks_in_vis", [None, 0.3])
@pytest.mark.parametrize("thresh", [0.5, 0.9])
def test_hard_nms_agrees_with_the_transcription(case, thresh, oks_in_vis):
    keep, score, rank, oks = R.pose_nms_ref(*_args(case), oks_thresh=thresh, in_vis_thre=IN_VIS, oks_in_vis_thre=oks_in_vis,
                                            return_oks=True)
    sizes, worst = set(), 0.0
    for a, b, db in _frames(case):
        n = b - a
        sizes.add(n)
        want_score = np.array([p["score"] for p in db])
        assert np.array_equal(score[a:b].view(np.int64), want_score.view(np.int64))      # bit for bit
        assert np.array_equal(np.argsort(rank[a:b]), want_score.argsort(kind="stable")[::-1])
        kpts = np.array([p["keypoints"].flatten() for p in db])
        areas = np.array([p["area"] for p in db])
        for g in range(n):
            row = R.hrnet_oks_iou(kpts[g], kpts, areas[g], areas, None, oks_in_vis)
            assert np.array_equal(np.isnan(row), np.isnan(oks[a + g, :n]))
            # np.sum adds the 17 terms <= 1 in another order than left to right: at most 17 roundings of 2^-53 each way
            worst = max(worst, np.abs(row - oks[a + g, :n])[~np.isnan(row)].max(initial=0.0))
        want = np.zeros(n, bool)
        want[R.hrnet_oks_nms(db, thresh, None, oks_in_vis)] = True
        assert np.array_equal(keep[a:b], want)
    print("largest OKS difference", worst)
    assert worst <= 1e-13
    assert {1, 2, 3, 63, 64} <= sizes


@pytest.mark.parametrize("soft_type", ["gaussian", "linear"])
def test_soft_nms_agrees_with_the_transcription(case, soft_type):
    settings = dict(oks_thresh=0.5, in_vis_thre=IN_VIS, soft=True, soft_type=soft_type)
    keep, score, rank, oks = R.input_conditions(*_args(case), **settings)
    for a, b, db in _frames(case):
        n = b - a
        # the two OKS differ by <= 1e-13 (above).  A gaussian factor exp(-oks^2 / 0.5) then differs by <= 4e-13 relative;
        # a linear factor 1 - oks by <= 1e-13 / (1 - oks), which the frame's closest OKS below 1 bounds; <= 20 factors each
        o = oks[a:b, :n]
        near = o[(o >= 0.5) & (o < 1.0)]
        tol = 20 * (4e-13 if soft_type == "gaussian" else 1e-13 / (1.0 - near.max(initial=0.5)))
        want_keep, want_taken = R.hrnet_soft_oks_nms(db, 0.5, None, None, soft_type)
        assert len(want_keep) == min(n, 20) == keep[a:b].sum()
        got = np.argsort(np.where(rank[a:b] >= 0, rank[a:b], n + 1), kind="stable")[:len(want_keep)]
        # who is taken, and in which order.  Once a person with NaN coordinates is taken every remaining score is NaN: the
        # contract orders such ties by person index, the transcription's re-sort by position in its current order, so
        # there the two agree on the set (docstring of hrnet_soft_oks_nms)
        if np.isnan(want_taken).sum() > 1:
            assert np.array_equal(np.sort(got), np.sort(want_keep))
            continue
        assert np.array_equal(got, want_keep)
        assert np.array_equal(np.sort(rank[a:b][keep[a:b]]), np.arange(len(want_keep)))
        s = score[a:b][want_keep]
        assert np.array_equal(np.isnan(s), np.isnan(want_taken))
        m = ~np.isnan(s)
        assert (np.abs(s[m] - want_taken[m]) <= tol * np.abs(want_taken[m])).all()


def _one_frame(scores, xy=None, area=1e4, **settings):
    """A frame whose persons have the given person scores (all 17 maxvals 1, box score = the score)."""
    n = len(scores)
    preds = np.zeros((n, 17, 2), np.float32)
    preds[:, :, 0] = np.arange(n)[:, None] * 1000.0 if xy is None else xy
    args = (np.array([0, n], np.int32), np.arange(n, dtype=np.int32), preds, np.ones((n, 17), np.float32),
            np.asarray(scores, np.float64), np.full(n, area))
    return R.pose_nms_ref(*args, **settings)


def test_tie_and_nan_rules_on_hand_made_frames():
    # equal scores: the later person first; a NaN score before every number, several NaNs by the same rule
    keep, score, rank = _one_frame([0.5, 0.7, 0.5, np.nan, 0.7, np.nan], oks_thresh=0.5)
    assert keep.all() and rank.tolist() == [5, 3, 4, 1, 2, 0]
    # the same order decides who survives: persons 0 and 2 share a pose and a score, the later one is kept
    keep, _, rank = _one_frame([0.5, 0.9, 0.5], xy=np.array([0.0, 500.0, 0.0])[:, None], oks_thresh=0.5)
    assert keep.tolist() == [False, True, True] and rank.tolist() == [2, 0, 1]
    # a NaN OKS kills (NaN <= thresh is false), also at a threshold nothing finite exceeds
    keep, _, _ = _one_frame([0.9, 0.5, 0.4], xy=np.array([0.0, np.nan, 900.0])[:, None], oks_thresh=1.0)
    assert keep.tolist() == [True, False, True]
    # ... unless the NaN person leads: it is kept and kills everybody after it
    keep, _, _ = _one_frame([0.5, 0.9, 0.4], xy=np.array([0.0, np.nan, 900.0])[:, None], oks_thresh=1.0)
    assert keep.tolist() == [False, True, False]
    # soft: ties are taken later person first, each with the score it has then; max_dets bounds the kept
    keep, score, rank = _one_frame([0.5, 0.5, 0.5], oks_thresh=0.5, soft=True, max_dets=2)
    assert rank.tolist() == [-1, 1, 0] and keep.tolist() == [False, True, True]
    assert score[2] == 0.5 and score[1] == 0.5 * math.exp(-0.0)
    # an exact duplicate decays by exp(-1 / thresh) (gaussian) or to 0 (linear: 1 - 1)
    xy = np.array([0.0, 0.0])[:, None]
    _, score, _ = _one_frame([0.9, 0.8], xy=xy, oks_thresh=0.5, soft=True)
    assert score[0] == 0.9 and score[1] == 0.8 * np.exp(-1.0 / 0.5)
    _, score, _ = _one_frame([0.9, 0.8], xy=xy, oks_thresh=0.5, soft=True, soft_type="linear")
    assert score.tolist() == [0.9, 0.0]


def test_placeholder_is_kept_and_suppresses_nobody():
    preds = np.zeros((1, 17, 2), np.float32)
    args = (np.array([0, 2, 3], np.int32), np.array([-1, 0, -1], np.int32), preds, np.ones((1, 17), np.float32),
            np.array([0.8]), np.array([0.0]))
    for soft in (False, True):
        keep, score, rank, oks = R.pose_nms_ref(*args, oks_thresh=0.5, soft=soft, return_oks=True)
        assert keep.all() and score.tolist() == [0.0, 0.8, 0.0] and rank.tolist() == [1, 0, 0]
        assert not oks.any() or oks[1, 1] == 1.0 and np.count_nonzero(oks) == 1


def test_c_entry_point_refuses_bad_arguments_without_a_gpu():
    L = hip.lib()
    sig = (ctypes.c_double * 17)(*R.COCO_SIGMAS)
    assert L.otp_pose_nms(None, None, None, None, None, None, sig, 0.0, 0.9, math.nan, 0, 20, None, None, None, None,
                          1, 1, 1, None) == -1
    one = ctypes.c_void_p(8)                                         # never dereferenced: the checks come first
    tail = (one, one, one, None, 1, 1, 1, None)
    assert L.otp_pose_nms(one, one, one, one, one, one, None, 0.0, 0.9, math.nan, 0, 20, *tail) == -1
    assert L.otp_pose_nms(one, one, one, one, one, one, sig, 0.0, 0.0, math.nan, 0, 20, *tail) == -1
    assert L.otp_pose_nms(one, one, one, one, one, one, sig, 0.0, math.inf, math.nan, 0, 20, *tail) == -1
    assert L.otp_pose_nms(one, one, one, one, one, one, sig, 0.0, 0.9, math.nan, 3, 20, *tail) == -1
    assert L.otp_pose_nms(one, one, one, one, one, one, sig, 0.0, 0.9, math.nan, 1, 0, *tail) == -1
    assert L.otp_pose_nms(one, one, one, one, one, one, sig, 0.0, 0.9, math.nan, 0, 20, one, one, one, None, 0, 1, 1, None) == -1
    bad = (ctypes.c_double * 17)(*([0.05] * 16 + [0.0]))
    assert L.otp_pose_nms(one, one, one, one, one, one, bad, 0.0, 0.9, math.nan, 0, 20, *tail) == -1


def test_from_cfg_reads_the_posetrack_settings():
    shared = {"NMS_THRE": 1.0, "OKS_THRE": 0.9, "SOFT_NMS": False, "POST_PROCESS": True}
    pt18 = CfgNode({"VAL": dict(shared, IN_VIS_THRE=0.1), "TEST": dict(shared, IN_VIS_THRE=0.1)})       # Base_PoseTrack18.yaml
    pt17 = CfgNode({"VAL": dict(shared, IN_VIS_THRE=0.2), "TEST": dict(shared, IN_VIS_THRE=0.2, SOFT_NMS=True)})
    for cfg, vis in ((pt18, 0.1), (pt17, 0.2)):
        for phase in ("validate", "test"):
            nms = PE.PoseNMS.from_cfg(cfg, phase)
            assert (nms.oks_thresh, nms.in_vis_thre, nms.max_dets, nms.oks_in_vis_thre) == (0.9, vis, 20, None)
            assert nms.soft == (cfg is pt17 and phase == "test") and nms.soft_type == "gaussian"
            assert nms.sigmas == tuple(R.COCO_SIGMAS.tolist())
    assert PE.PoseNMS.from_cfg(CfgNode({"VAL": {"OKS_THRE": 0.9}, "TEST": {"OKS_THRE": 0.9, "POST_PROCESS": False}}),
                               "validate") is None
    assert PE.PoseNMS.from_cfg(CfgNode({"TEST": {"OKS_THRE": 0.9, "POST_PROCESS": False}}), "test") is None
    assert PE.PoseNMS.from_cfg(CfgNode({}), "validate") is None


def test_add_needs_an_area_when_the_evaluator_has_an_nms():
    frames = S.posetrack_eval_case(12, 3)[0]
    preds, maxvals = torch.zeros(2, 17, 2), torch.ones(2, 17, 1)
    ev = PE.PoseTrackEvaluator(frames, nms=PE.PoseNMS(oks_thresh=0.9))
    with pytest.raises(ValueError, match="area"):
        ev.add(preds, maxvals, [0.9, 0.8], [0, 0])
    with pytest.raises(ValueError):
        ev.add(preds, maxvals, [0.9, 0.8], [0, 0], area=[1.0])
    ev.add(preds, maxvals, [0.9, 0.8], [0, 0], area=[100.0, 50.0])
    scale = np.array([[0.5, 0.75], [1.1, 1.3]], np.float32)
    ev.add(preds, maxvals, [0.9, 0.8], [0, 0], scale=scale)
    want = (scale.astype(np.float64) * 200.0).prod(1)
    assert ev._area[1].dtype == torch.float64 and np.array_equal(ev._area[1].numpy(), want)
    PE.PoseTrackEvaluator(frames).add(preds, maxvals, [0.9, 0.8], [0, 0])          # without an NMS nothing changes
