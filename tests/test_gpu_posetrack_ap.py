"""PoseTrack AP on the GPU: ``ops.pose_assign`` bit for bit against the vectors of the reference's evaluator
(tests/golden/posetrack_ap.npz) and, on a seeded case of about 3 000 frames, against the numpy restatement
(tests/posetrack_ap_ref.py); ``ops.ap_curve`` / ``PoseTrackEvaluator.summarize`` within 1e-9 percentage points (the bound
derived in tests/test_posetrack_ap_host.py: the order of the final sum over at most 2^16 terms).  Every frame and joint is
compared; the input conditions (a)-(d) are asserted on the generated data and exclude nothing."""
import os

import numpy as np
import pytest
import torch

from otpose_amd import OTPose, ops, posetrack_eval as PE, synthetic as S, tiny_cfg
from otpose_amd import crop as C
from tests import posetrack_ap_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posetrack_ap.npz")
GT_KEYS = ("gt_off", "gt_xy", "gt_has", "gt_head", "poly_off", "vert_off", "vert_xy")
TOL = 1e-9


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _host_args(pr_off, pr_sample, preds, box, g):
    return [pr_off, pr_sample, preds[:, :, :2], preds[:, :, 2:], box] + [g[k] for k in GT_KEYS]


def _device(args):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]


@pytest.fixture(scope="module")
def large():
    """About 3 000 frames; two frames at the kernel's person limits, three asked to carry a 64-vertex ignore polygon
    (a frame whose ground truth is empty is dropped with its polygon)."""
    frames, preds, box, fid = S.posetrack_eval_case(3000, 7, crowded=(5, 1500), big_polygon=(9, 77, 1500))
    g = PE.pack_ground_truth(frames)
    pr_off, pr_sample = PE.pack_predictions(g["frame_map"], fid, len(g["kept"]))
    args = _host_args(pr_off, pr_sample, preds, box, g)
    assert np.diff(pr_off).max() == ops.POSEVAL_MAX_PR and np.diff(g["gt_off"]).max() == ops.POSEVAL_MAX_GT
    assert np.diff(g["vert_off"]).max() == 64
    most = R.input_conditions(*args)                                 # (a) - (d)
    assert most <= 2 ** 16
    return frames, preds, box, fid, g, args


def test_pose_assign_matches_the_reference_bit_for_bit(gold):
    args = _host_args(gold["pr_off"], gold["pr_sample"], gold["preds"], gold["box_score"], gold)
    labels, scores, ngt = ops.pose_assign(*_device(args))
    assert labels.dtype == torch.int8 and scores.dtype == torch.float64 and ngt.dtype == torch.int32
    assert np.array_equal(labels.cpu().numpy(), gold["labels"])
    assert np.array_equal(scores.cpu().numpy().view(np.int64), gold["scores"].view(np.int64))
    assert np.array_equal(ngt.cpu().numpy(), gold["nGTall"])


def test_ap_curve_and_summarize_match_the_reference(gold):
    args = _host_args(gold["pr_off"], gold["pr_sample"], gold["preds"], gold["box_score"], gold)
    labels, scores, ngt = ops.pose_assign(*_device(args))
    lab, off, sc = ops.sort_entries(labels, scores)
    out, prec, rec = ops.ap_curve(lab, off, ngt.sum(0, dtype=torch.int64), return_curve=True)
    out = out.cpu().numpy()
    for c, want in enumerate((gold["apAll"], gold["preAll"], gold["recAll"])):
        got = PE.with_mean(out[:, c])
        print(("ap", "precision", "recall")[c], "max |diff| =", np.abs(got - want).max())
        assert np.abs(got - want).max() <= TOL
    # the curve itself: exact divisions of the running count
    off_h, lab_h = off.cpu().numpy(), lab.cpu().numpy()
    total = gold["nGTall"].sum(0).astype(np.float64)
    for j in range(15):
        l = lab_h[off_h[j]:off_h[j + 1]]
        npos = np.cumsum(l == 1).astype(np.float64)
        assert np.array_equal(prec.cpu().numpy()[off_h[j]:off_h[j + 1]], npos / np.arange(1, l.size + 1))
        assert np.array_equal(rec.cpu().numpy()[off_h[j]:off_h[j + 1]], npos / total[j])
        s = sc.cpu().numpy()[off_h[j]:off_h[j + 1]]
        assert (np.diff(s) <= 0).all()
    frames = S.posetrack_eval_case(int(gold["frames"]), int(gold["seed"]))[0]
    ev = PE.PoseTrackEvaluator(frames)
    p = torch.from_numpy(gold["preds"]).cuda()
    ev.add(p[:, :, :2], p[:, :, 2:], gold["box_score"], gold["frame_id"])
    res = ev.summarize()
    for k, want in (("ap", gold["apAll"]), ("precision", gold["preAll"]), ("recall", gold["recAll"])):
        assert res[k].shape == (16,) and res[k].dtype == np.float64
        assert np.abs(res[k] - want).max() <= TOL
    assert list(res["table"]) == list(PE.TABLE_KEYS)
    assert np.abs(np.array(list(res["table"].values())) - gold["table"]).max() <= TOL
    assert res["table"]["Mean"] == res["ap"][15]


def test_large_case_matches_the_restatement(large):
    frames, preds, box, fid, g, args = large
    want_l, want_s, want_n = R.pose_assign_ref(*args)
    dev = _device(args)
    labels, scores, ngt = ops.pose_assign(*dev)
    assert np.array_equal(labels.cpu().numpy(), want_l)
    assert np.array_equal(scores.cpu().numpy().view(np.int64), want_s.view(np.int64))
    assert np.array_equal(ngt.cpu().numpy(), want_n)
    lab, off, _ = ops.sort_entries(labels, scores)
    out = ops.ap_curve(lab, off, ngt.sum(0, dtype=torch.int64))
    want = R.ap_curve_ref(want_l, want_s, want_n)
    for c in range(3):
        got = PE.with_mean(out.cpu().numpy()[:, c])
        print(("ap", "precision", "recall")[c], "max |diff| =", np.abs(got - want[c]).max())
        assert np.isfinite(want[c]).all() and np.abs(got - want[c]).max() <= TOL
    # two runs, identical bytes
    labels2, scores2, ngt2 = ops.pose_assign(*dev)
    out2 = ops.ap_curve(*ops.sort_entries(labels2, scores2)[:2], ngt2.sum(0, dtype=torch.int64))
    assert torch.equal(labels, labels2) and torch.equal(scores.view(torch.int64), scores2.view(torch.int64))
    assert torch.equal(ngt, ngt2) and torch.equal(out.view(torch.int64), out2.view(torch.int64))


def test_ragged_batches_equal_one_add(large):
    frames, preds, box, fid, g, _ = large
    p = torch.from_numpy(preds).cuda()
    one = PE.PoseTrackEvaluator(g)
    one.add(p[:, :, :2], p[:, :, 2:], box, fid)
    a = one.summarize()
    many = PE.PoseTrackEvaluator(g)
    cuts = [0, 1, 18, 19, 700, 5000, 5001, preds.shape[0]]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        many.add(p[lo:hi, :, :2].contiguous(), p[lo:hi, :, 2:].contiguous(), torch.from_numpy(box[lo:hi]), fid[lo:hi])
    b = many.summarize()
    for k in ("ap", "precision", "recall"):
        assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64))
    assert a["table"] == b["table"]
    many.reset()
    with pytest.raises(RuntimeError):
        many.summarize()


def test_limits_are_checked_on_the_host(gold):
    args = _host_args(gold["pr_off"], gold["pr_sample"], gold["preds"], gold["box_score"], gold)
    n = ops.POSEVAL_MAX_PR + 1
    over = list(args)
    over[0] = np.array([0, n] + [n] * (len(gold["kept"]) - 1), np.int32)
    over[1] = np.zeros(n, np.int32)
    with pytest.raises(ValueError, match="limit"):
        ops.pose_assign(*_device(over))
    bad = list(args)
    bad[1] = np.where(gold["pr_sample"] >= 0, gold["pr_sample"] + gold["preds"].shape[0], -1).astype(np.int32)
    with pytest.raises(ValueError):
        ops.pose_assign(*_device(bad))
    with pytest.raises(NotImplementedError):
        ops.pose_assign(*[torch.from_numpy(np.ascontiguousarray(a)) for a in args])


def test_predict_to_summarize_end_to_end():
    """Predictions of ``OTPose.predict`` on a small synthetic pool go through add / summarize; the result equals the numpy
    restatement on the same predictions copied to the host."""
    cfg = tiny_cfg(8, (64, 96))
    model = OTPose(cfg)
    S.fill_synthetic_(model)
    model = model.cuda().eval()
    w_img, h_img = cfg.MODEL.IMAGE_SIZE
    rng = np.random.RandomState(4)
    pool = torch.from_numpy(rng.randint(0, 256, (9, 90, 130, 3)).astype(np.uint8)).cuda()
    boxes = [[30.0, 10.0, 40.0, 60.0], [70.5, 40.2, 50.0, 45.0], [10.0, 20.0, 60.0, 50.0], [55.0, 5.0, 45.0, 70.0]]
    c, s = C.box_to_center_scale(boxes, w_img / h_img, 1.25)
    fi = rng.randint(0, 9, (4, 5))
    _, margin = S.synthetic_clip(4, (w_img, h_img))
    with torch.no_grad():
        preds, maxvals = model.predict(pool, fi, c, s, margin)
    p = preds.cpu().numpy().astype(np.float64)

    def person(sample, shift, joints):
        q = p[sample][list(PE.COCO_OF_OFFICIAL)] + shift
        return {"annopoints": [{"point": [{"id": [k], "x": [float(q[k, 0])], "y": [float(q[k, 1])]} for k in joints]}],
                "x1": [10.0], "y1": [10.0], "x2": [22.0], "y2": [26.0]}               # head size 0.6 * 20 = 12 px

    frames = [{"annorect": [person(0, 1.0, range(15)), person(1, 30.0, range(0, 15, 2))]},
              {"annorect": []},
              {"annorect": [person(2, 2.5, range(15))],
               "ignore_regions": [{"point": [{"x": [float(p[3, 0, 0] + dx)], "y": [float(p[3, 0, 1] + dy)]}
                                             for dx, dy in ((-3, -3), (3, -3), (3, 3), (-3, 3))]}]},
              {"annorect": [person(3, 0.5, range(15))]}]
    frame_id = np.array([0, 0, 2, 2])                                 # frame 3 gets the placeholder person
    box = np.array([0.9, 0.8, 0.7, 0.6])
    ev = PE.PoseTrackEvaluator(frames)
    ev.add(preds[:3], maxvals[:3], box[:3], frame_id[:3])
    ev.add(preds[3:], maxvals[3:], box[3:], frame_id[3:])
    res = ev.summarize()
    g = ev.gt
    pr_off, pr_sample = PE.pack_predictions(g["frame_map"], frame_id, len(g["kept"]))
    args = [pr_off, pr_sample, preds.cpu().numpy(), maxvals.cpu().numpy(), box] + [g[k] for k in GT_KEYS]
    R.input_conditions(*args)
    labels, scores, ngt = ev.assign()[:3]
    want_l, want_s, want_n = R.pose_assign_ref(*args)
    assert np.array_equal(labels.cpu().numpy(), want_l) and np.array_equal(scores.cpu().numpy(), want_s)
    assert np.array_equal(ngt.cpu().numpy(), want_n)
    assert (want_l == 1).any() and (want_l == 0).any() and (want_l == -1).any()
    want = R.ap_curve_ref(want_l, want_s, want_n)
    for k, w in zip(("ap", "precision", "recall"), want):
        assert np.abs(res[k] - w).max() <= TOL
    assert res["table"] == PE.cum_table(want[0]) or np.abs(
        np.array(list(res["table"].values())) - np.array(list(PE.cum_table(want[0]).values()))).max() <= TOL


def test_joint_with_entries_but_no_annotated_ground_truth_gives_the_reference_nan():
    """compute_rpc divides by nGT = 0 (utils/evaluate.py:698): recall is NaN (no positive) or inf, vocap's sum NaN, and
    compute_metrics' mean skips the joint (:724-729).  Joint 3 is annotated nowhere but predicted everywhere; joint 4 is
    fed to the kernel with a positive label and nGT = 0 directly."""
    rng = np.random.RandomState(11)
    joints = [k for k in range(15) if k != 3]
    frames, preds = [], np.zeros((6, 17, 3), np.float32)
    for f in range(3):
        pose = rng.uniform(100, 900, (15, 2))
        frames.append({"annorect": [{"annopoints": [{"point": [{"id": [k], "x": [float(pose[k, 0])], "y": [float(pose[k, 1])]}
                                                               for k in joints]}],
                                     "x1": [0.0], "y1": [0.0], "x2": [30.0], "y2": [40.0]}]})
        for d in range(2):
            preds[2 * f + d, list(PE.COCO_OF_OFFICIAL), :2] = pose + (2.0 if d == 0 else 200.0)
            preds[2 * f + d, :, 2] = rng.uniform(0.1, 1.0, 17)
    box, fid = rng.uniform(0.3, 1.0, 6), np.repeat(np.arange(3), 2)
    ev = PE.PoseTrackEvaluator(frames)
    p = torch.from_numpy(preds).cuda()
    ev.add(p[:, :, :2], p[:, :, 2:], box, fid)
    res = ev.summarize()
    g = ev.gt
    pr_off, pr_sample = PE.pack_predictions(g["frame_map"], fid, 3)
    args = _host_args(pr_off, pr_sample, preds, box, g)
    R.input_conditions(*args)
    want_l, want_s, want_n = R.pose_assign_ref(*args)
    assert want_n[:, 3].sum() == 0 and (want_l[:, 3] == 0).all() and (want_l[:, 0] == 1).any()
    want = R.ap_curve_ref(want_l, want_s, want_n)
    assert np.isnan(want[0][3]) and np.isnan(want[2][3]) and want[1][3] == 0.0 and np.isfinite(want[0][15])
    for k, w in zip(("ap", "precision", "recall"), want):
        assert np.array_equal(np.isnan(res[k]), np.isnan(w))
        assert np.abs(res[k] - w)[~np.isnan(w)].max() <= TOL
    assert np.isfinite(res["table"]["Mean"]) and np.isnan(res["table"]["Hip"])      # Hip = mean(right_hip, left_hip = 3)
    # a positive label under nGT = 0: recall is inf, the sentinel term (1 - inf) * 0 makes the area NaN, as numpy does
    lab = torch.tensor([0, 0, 0, 1, 0, 1, 1, 0], dtype=torch.int8).cuda()
    off = torch.tensor([0, 3, 5, 8], dtype=torch.int64).cuda()
    out = ops.ap_curve(lab, off, torch.tensor([0, 0, 4], dtype=torch.int64).cuda()).cpu().numpy()
    assert np.isnan(out[0, 0]) and out[0, 1] == 0.0 and np.isnan(out[0, 2])
    assert np.isnan(out[1, 0]) and out[1, 1] == 50.0 and np.isinf(out[1, 2])
    # joint 2: precision 1, 1, 2/3 -> mpre 1, 1, 2/3; recall .25, .5, .5 -> area .25 + .25
    assert out[2].tolist() == [50.0, (2.0 / 3.0) * 100.0, 50.0]


def test_argument_types_are_checked_before_use(gold):
    args = _device(_host_args(gold["pr_off"], gold["pr_sample"], gold["preds"], gold["box_score"], gold))
    for i in (3, 0, 11):
        bad = list(args)
        bad[i] = bad[i].cpu().numpy()
        with pytest.raises(TypeError):
            ops.pose_assign(*bad)
    bad = list(args)
    bad[10] = torch.zeros(0, dtype=torch.int32).cuda()
    with pytest.raises(ValueError):
        ops.pose_assign(*bad)
