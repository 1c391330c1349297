"""Host side of the PoseTrack AP evaluation: the numpy restatement (tests/posetrack_ap_ref.py) against the vectors the
reference's evaluator produced (tests/golden/posetrack_ap.npz, recipe make_golden_posetrack_ap.py), the packing of
``otpose_amd.posetrack_eval``, and the argument checks.  No GPU needed.

Labels, scores and nGT are compared exactly on every frame and joint.  AP / precision / recall are compared to 1e-9
percentage points: labels and the divisions are exact, only the final sum over at most 2^16 terms <= 1 differs in order from
numpy's pairwise sum, which bounds the difference by 2^16 * 1.1e-16 * 100 ~ 7e-10 (the tests keep every joint at or below
2^16 entries)."""
import os

import numpy as np
import pytest
import torch

from otpose_amd import hip, posetrack_eval as PE, synthetic as S
from tests import posetrack_ap_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posetrack_ap.npz")
GT_KEYS = ("gt_off", "gt_xy", "gt_has", "gt_head", "poly_off", "vert_off", "vert_xy")
TOL = 1e-9


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def packed_args(g):
    return [g["pr_off"], g["pr_sample"], g["preds"][:, :, :2], g["preds"][:, :, 2:], g["box_score"]] + [g[k] for k in GT_KEYS]


def test_restatement_matches_the_reference_on_every_frame_and_joint(gold):
    labels, scores, ngt = R.pose_assign_ref(*packed_args(gold))
    assert labels.dtype == np.int8 and labels.shape == gold["labels"].shape
    assert np.array_equal(labels, gold["labels"])
    assert np.array_equal(scores, gold["scores"])                    # exact float64
    assert np.array_equal(ngt, gold["nGTall"])
    for f in range(len(gold["kept"])):                               # nothing left out: every frame has its rows
        a, b = gold["pr_off"][f], gold["pr_off"][f + 1]
        assert b > a
    ap, pre, rec = R.ap_curve_ref(labels, scores, ngt)
    most = max((labels[:, j] >= 0).sum() for j in range(15))
    assert 0 < most <= 2 ** 16
    for got, want in ((ap, gold["apAll"]), (pre, gold["preAll"]), (rec, gold["recAll"])):
        assert got.shape == (16,) and np.isfinite(want).all()
        assert np.abs(got - want).max() <= TOL, np.abs(got - want).max()
    table = PE.cum_table(ap)
    assert list(table) == ["Head", "Shoulder", "Elbow", "Wrist", "Hip", "Knee", "Ankle", "Mean"]
    assert np.abs(np.array(list(table.values())) - gold["table"]).max() <= TOL


def test_input_conditions_hold_on_the_golden(gold):
    assert R.input_conditions(*packed_args(gold)) <= 2 ** 16


def test_cum_table_is_getcum():
    v = np.arange(16, dtype=np.float64) ** 2 + 0.25
    t = PE.cum_table(v)
    want = [(v[14] + v[12] + v[13]) / 3, (v[8] + v[9]) / 2, (v[7] + v[10]) / 2, (v[6] + v[11]) / 2, (v[2] + v[3]) / 2,
            (v[1] + v[4]) / 2, (v[0] + v[5]) / 2, v[15]]
    assert list(t.values()) == want
    m = PE.with_mean(np.r_[np.arange(14.0), np.nan])
    assert m.shape == (16,) and m[15] == np.arange(14.0).mean()      # the mean skips NaN joints (compute_metrics)


def test_pack_ground_truth_drops_frames_and_builds_the_offsets(gold):
    frames, preds, box, fid = S.posetrack_eval_case(int(gold["frames"]), int(gold["seed"]))
    assert np.array_equal(preds, gold["preds"]) and np.array_equal(box, gold["box_score"])
    assert np.array_equal(fid, gold["frame_id"])
    g = PE.pack_ground_truth(frames)
    assert g["num_frames"] == int(gold["frames"])
    assert np.array_equal(g["kept"], gold["kept"]) and len(g["kept"]) < g["num_frames"]
    assert (g["frame_map"][g["kept"]] == np.arange(len(g["kept"]))).all() and (g["frame_map"] < 0).sum() == \
        g["num_frames"] - len(g["kept"])
    for k in GT_KEYS:
        assert g[k].dtype == gold[k].dtype and np.array_equal(g[k], gold[k]), k
    pr_off, pr_sample = PE.pack_predictions(g["frame_map"], fid, len(g["kept"]))
    assert pr_off.dtype == np.int32 and np.array_equal(pr_off, gold["pr_off"])
    assert np.array_equal(pr_sample, gold["pr_sample"])
    # arrival order within a frame survives interleaved batches
    order = np.random.RandomState(0).permutation(fid.size)
    _, shuffled = PE.pack_predictions(g["frame_map"], fid[order], len(g["kept"]))
    for f in range(len(g["kept"])):
        got = shuffled[pr_off[f]:pr_off[f + 1]]
        if got[0] >= 0:
            assert (np.diff(got) > 0).all() and (fid[order][got] == g["kept"][f]).all()


def _annolist_arrays(frames):
    off, pts, xy, sc, rs, tr = [0], [], [], [], [], []
    for fr in frames:
        for rect in fr["annorect"]:
            p = rect["annopoints"][0]["point"]
            assert [q["id"][0] for q in p] == list(range(len(p)))
            a, s = np.zeros((15, 2)), np.zeros(15)
            for q in p:
                a[q["id"][0]] = (q["x"][0], q["y"][0])
                s[q["id"][0]] = q["score"][0]
            pts.append(len(p)), xy.append(a), sc.append(s), rs.append(float(rect["score"][0])), tr.append(rect["track_id"][0])
        off.append(len(pts))
    return off, pts, np.asarray(xy), np.asarray(sc), np.asarray(rs), tr


def test_annolist_equals_the_frames_the_reference_wrote(gold):
    frames, preds, box, fid = S.posetrack_eval_case(int(gold["frames"]), int(gold["seed"]))
    ev = PE.PoseTrackEvaluator(frames)
    p = torch.from_numpy(preds)
    cut = preds.shape[0] // 3
    ev.add(p[:cut, :, :2], p[:cut, :, 2:], box[:cut], fid[:cut])
    ev.add(p[cut:, :, :2], p[cut:, :, 2:], torch.from_numpy(box[cut:]), torch.from_numpy(fid[cut:]))
    off, pts, xy, sc, rs, tr = _annolist_arrays(ev.annolist())
    assert off == gold["ann_off"].tolist() and pts == gold["ann_points"].tolist() and tr == gold["ann_track"].tolist()
    assert np.array_equal(xy, gold["ann_xy"]) and np.array_equal(sc, gold["ann_score"])      # exact floats
    assert np.array_equal(rs, gold["ann_rect_score"])
    assert 1 in pts                                                   # a placeholder person is among them
    ev.reset()
    with pytest.raises(RuntimeError):
        ev.annolist()


def test_argument_checks():
    frames, preds, box, fid = S.posetrack_eval_case(12, 3)
    ev = PE.PoseTrackEvaluator(frames)
    p = torch.from_numpy(preds)
    with pytest.raises(ValueError):
        ev.add(p[:2, :, :2], p[:2, :, 2:], box[:2], [0, 12])          # frame_id out of range
    with pytest.raises(ValueError):
        ev.add(p[:2, :, :2], p[:2, :, 2:], box[:2], [-1, 0])
    with pytest.raises(ValueError):
        ev.add(p[:2, :, :2], p[:2, :, 2:], box[:3], [0, 1])
    with pytest.raises(ValueError):
        ev.add(p[:2, :, :2].double(), p[:2, :, 2:], box[:2], [0, 1])
    g = ev.gt
    f = int(g["kept"][0])
    with pytest.raises(ValueError, match="limit"):                    # over-limit predicted persons
        PE.pack_predictions(g["frame_map"], np.full(PE.MAX_PR + 1, f), len(g["kept"]))
    PE.pack_predictions(g["frame_map"], np.full(PE.MAX_PR, f), len(g["kept"]))
    person = {"annopoints": [{"point": [{"id": [0], "x": [1.0], "y": [2.0]}]}], "x1": [0.0], "y1": [0.0], "x2": [3.0],
              "y2": [4.0]}
    with pytest.raises(ValueError, match="limit"):                    # over-limit ground-truth persons
        PE.pack_ground_truth([{"annorect": [person] * (PE.MAX_GT + 1)}])
    assert PE.pack_ground_truth([{"annorect": [person] * PE.MAX_GT}])["gt_off"].tolist() == [0, PE.MAX_GT]
    bad = {"annopoints": [{"point": [{"id": [15], "x": [1.0], "y": [2.0]}]}], "x1": [0.0], "y1": [0.0], "x2": [3.0], "y2": [4.0]}
    with pytest.raises(ValueError):
        PE.pack_ground_truth([{"annorect": [bad]}])
    with pytest.raises(ValueError):
        PE.pack_ground_truth([{"annorect": [person], "ignore_regions": [{"point": [{"x": [0.0], "y": [0.0]}] * 2}]}])
    assert PE.MAX_PR >= 64 and PE.MAX_GT >= 64
    # the operators have no CPU path
    ev.add(p[:, :, :2], p[:, :, 2:], box, fid)
    with pytest.raises(NotImplementedError):
        ev.summarize()


def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    L = hip.lib()
    assert L.otp_pose_assign(*([None] * 12), 0.5, None, None, None, 1, 1, 1, 1, None) == -1
    assert L.otp_ap_curve(None, None, None, None, None, None, 15, None) == -1
    one = np.zeros(64, np.int64)
    ptr = one.ctypes.data
    assert L.otp_pose_assign(*([ptr] * 12), 0.5, ptr, ptr, ptr, -1, 1, 1, 1, None) == -1          # negative counts
    assert L.otp_pose_assign(*([ptr] * 12), 0.5, ptr, ptr, ptr, 1, 0, 1, 1, None) == -1
    assert L.otp_pose_assign(*([ptr] * 12), 0.5, ptr, ptr, None, 1, 1, 1, 1, None) == -1
    assert L.otp_ap_curve(ptr, ptr, ptr, ptr, None, None, 0, None) == -1
    assert L.otp_ap_curve(ptr, ptr, ptr, None, None, None, 15, None) == -1
