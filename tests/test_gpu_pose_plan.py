"""``ops.pose_plan`` (csrc/plan.hip) against the numpy restatement of the host recipe (tests/pose_plan_ref.py): every
output equal bit for bit except ``M``, whose closed form is held to ``pose_plan_ref.M_TOL`` of the LAPACK solve - and to
crops that equal the host matrices' crops exactly."""
import numpy as np
import pytest
import torch

from otpose_amd import ops
from tests import pose_plan_ref as R

pytestmark = pytest.mark.gpu
SIZE = (48, 64)
AR = SIZE[0] / SIZE[1]
EXACT = ("center", "scale", "frame_idx", "margin", "box_score", "person_slot", "pr_off")


def _main_case():
    """S = 7, K = 4: two sequences (3 and 4 frames) share the pool, slots 0 and 6 are halo, frame 3 has no person."""
    rng = np.random.RandomState(11)
    S, K = 7, 4
    counts = np.array([0, 4, 1, 0, 3, 4, 2], np.int32)
    boxes = np.stack([rng.uniform(-10, 90, (S, K)), rng.uniform(-10, 60, (S, K)), rng.uniform(12, 70, (S, K)),
                      rng.uniform(12, 70, (S, K))], axis=2)
    boxes[1, 0] = [20.0, 30.0, 60.0, 20.0]          # wider than 3 : 4 -> heightened
    boxes[1, 1] = [50.5, 10.25, 15.0, 60.0]         # taller -> widened
    boxes[1, 2] = [-21.0, 5.0, 40.0, 30.0]          # center x exactly -1: not enlarged
    boxes[4, 0] = [30.0, 20.0, 30.0, 40.0]          # exactly 3 : 4 -> neither
    scores = rng.uniform(0.55, 1.0, (S, K)).astype(np.float32)
    scores[1, 3], scores[4, 1], scores[5, 0], scores[5, 2] = 0.1, 0.49, 0.5, 0.3      # 0.5 itself is kept
    scores[6] = 0.9                                  # halo: never a person, whatever the score
    for s in range(S):
        boxes[s, counts[s]:], scores[s, counts[s]:] = 0, 0
    fn = np.array([0, 1, 2, 0, 1, 2, 3], np.int32)
    nf = np.array([3, 3, 3, 4, 4, 4, 4], np.int32)
    return boxes, scores, counts, fn, nf


def _both(case, detect, max_persons, min_score=0.5, posetrack18=True):
    boxes, scores, counts, fn, nf = case
    want = R.pose_plan_ref(boxes, scores, counts, fn, nf, detect, min_score, AR, 1.25, SIZE, posetrack18, max_persons)
    got = ops.pose_plan(*[torch.from_numpy(a).cuda() for a in case], image_size=SIZE, max_persons=max_persons, detect=detect,
                        min_score=min_score, posetrack18=posetrack18)
    return got, want


def _check(got, want):
    assert int(got.total) == want["total"]
    for name in EXACT:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, name
        assert np.array_equal(g, want[name]), name
    err = np.abs(got.M.cpu().numpy() - want["M"]).max()
    print("max |M - crop_matrix| = %.3e (bound %.3e)" % (err, R.M_TOL))
    assert err <= R.M_TOL


@pytest.mark.parametrize("posetrack18", [True, False])
def test_plan_equals_the_host_recipe(posetrack18):
    case = _main_case()
    if not posetrack18:
        case = case[:3] + (case[3] + 1, case[4])
    got, want = _both(case, (1, 6), 12, posetrack18=posetrack18)
    assert want["total"] == 9 and want["pr_off"].tolist() == [0, 0, 3, 4, 4, 6, 9, 9]
    assert (want["frame_idx"][:9] == -1).sum() == 0 and (want["margin"][:9] == 0).any() and (want["margin"][:9] == 2).any()
    assert want["center"][2, 0] == -1 and want["scale"][2, 0] == np.float32(40 / 200)
    _check(got, want)


def test_plan_with_a_missing_halo_has_fallbacks_and_empty_slots():
    """The same pool with the numbers of slots 0 and 6 moved out of reach (not increasing towards their neighbours: other
    sequences) and frame 2 of the second video missing: prev / next fall back to the current frame, pprev / nnext become -1."""
    boxes, scores, counts, fn, nf = _main_case()
    fn = fn.copy()
    fn[0], fn[5], fn[6] = 2, 3, 0
    got, want = _both((boxes, scores, counts, fn, nf), (1, 6), 12)
    assert (want["frame_idx"][:9, 3] == -1).any() and (want["frame_idx"][:9, 4] == -1).any()
    assert (want["frame_idx"][:9, 1] == want["frame_idx"][:9, 0]).any() and (want["frame_idx"][:9, 2] == want["frame_idx"][:9, 0]).any()
    _check(got, want)


def test_plan_truncates_the_rows_but_not_the_total():
    got, want = _both(_main_case(), (1, 6), 5)
    assert want["total"] == 9 and want["pr_off"].tolist() == [0, 0, 3, 4, 4, 5, 5, 5] and got.center.shape == (5, 2)
    _check(got, want)
    got, want = _both(_main_case(), (1, 6), 0)                   # no rows at all: offsets and the total only
    assert int(got.total) == 9 and got.pr_off.cpu().tolist() == [0] * 8 and got.M.shape == (0, 2, 3)


def test_plan_scans_more_frames_than_one_pass_holds():
    rng = np.random.RandomState(5)
    S, K = 1300, 2
    counts = rng.randint(0, 2, S).astype(np.int32)
    boxes = np.stack([rng.uniform(0, 100, (S, K)), rng.uniform(0, 70, (S, K)), rng.uniform(10, 60, (S, K)),
                      rng.uniform(10, 60, (S, K))], axis=2)
    scores = rng.uniform(0.2, 1.0, (S, K)).astype(np.float32)
    case = (boxes, scores, counts, np.arange(S, dtype=np.int32), np.full(S, S, np.int32))
    got, want = _both(case, (0, S), 700, min_score=0.3)
    assert 500 < want["total"] < 700 and want["pr_off"][1024] < want["total"]      # persons on both sides of the pass border
    _check(got, want)


def test_crops_from_the_device_plan_equal_crops_from_the_host_plan():
    case = _main_case()
    got, want = _both(case, (1, 6), 12)
    pool = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (7, 96, 128, 3)).astype(np.uint8)).cuda()
    dev = ops.crop_clips(pool, got.frame_idx, got.M, size=SIZE)
    host = ops.crop_clips(pool, want["frame_idx"], want["M"], size=SIZE)
    assert dev.shape == (12, 15, 64, 48)
    if not torch.equal(dev, host):
        rows = sorted(set(torch.nonzero(dev != host)[:, 0].tolist()))
        M = got.M.cpu().numpy()
        for r in rows:
            s, k = [(s, k) for s in range(1, 6) for k in range(case[2][s]) if case[1][s, k] >= 0.5][r]
            d = M[r] - want["M"][r]
            print("row", r, "box", case[0][s, k].tolist(), "M - host M", d.tolist(),
                  "largest at coefficient", np.unravel_index(np.abs(d).argmax(), d.shape))
        pytest.fail(f"crops of rows {rows} differ between the device plan and the host plan")
    assert float(dev[9:].abs().max()) < 3 and torch.equal(dev[9:], dev[9:10].expand(3, -1, -1, -1))  # padding: empty frames
