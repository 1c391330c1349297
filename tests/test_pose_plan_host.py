"""The crop plan's numpy restatement (tests/pose_plan_ref.py) against hand-written windows, the closed form of the
rotation-0 crop matrix against ``crop.crop_matrix``, and the argument errors of ``ops.pose_plan`` / ``VideoPose`` - no GPU."""
import types

import numpy as np
import pytest
import torch

from otpose_amd import VideoPose, ops, tiny_cfg
from otpose_amd import crop as C
from tests import pose_plan_ref as R

AR, SIZE = 48 / 64, (48, 64)


def closed_form_matrix(center, scale, out_size):
    """(B, 2, 3) float64 as csrc/plan.hip forms it: crop_matrix's own float32 points at rotation 0 - src (cx, cy), (cx, y1),
    (x2, y1), dst (u0, v0), (u0, v1), (u2, v1) - then a = (u2 - u0) / (x2 - cx), d = (v0 - v1) / (cy - y1) and the
    translation in float64 (b = c = 0: each triangle is an axis-parallel right angle)."""
    f32, f64 = np.float32, np.float64
    c = np.asarray(center, f32).reshape(-1, 2)
    s = np.asarray(scale, f32).reshape(-1, 2)
    cx, cy = c[:, 0], c[:, 1]
    p1 = (s[:, 0] * f32(C.PIXEL_STD)).astype(f64) * -0.5
    y1 = (cy.astype(f64) + p1).astype(f32)
    x2 = cx + -(cy - y1)
    u0, v0 = f32(out_size[0] * 0.5), f32(out_size[1] * 0.5)
    v1 = f32(v0 + f32(out_size[0] * -0.5))
    u2 = f32(u0 + -f32(v0 - v1))
    a = (f64(u2) - f64(u0)) / (x2.astype(f64) - cx.astype(f64))
    d = (f64(v0) - f64(v1)) / (cy.astype(f64) - y1.astype(f64))
    M = np.zeros((len(c), 2, 3))
    M[:, 0, 0], M[:, 0, 2] = a, f64(u0) - a * cx.astype(f64)
    M[:, 1, 1], M[:, 1, 2] = d, f64(v0) - d * cy.astype(f64)
    return M


def _plan(fn, nf, persons_at, posetrack18=True, detect=None, min_score=0.0, max_persons=None, scores=None):
    """One box in each slot of ``persons_at`` (K = 1 unless ``scores`` (S, K) is given)."""
    S = len(fn)
    if scores is None:
        scores = np.zeros((S, 1), np.float32)
        counts = np.array([int(s in persons_at) for s in range(S)], np.int32)
        scores[list(persons_at)] = 0.9
    else:
        scores = np.asarray(scores, np.float32)
        counts = np.array(persons_at, np.int32)
    K = scores.shape[1]
    boxes = np.tile(np.array([10.0, 20.0, 30.0, 40.0]), (S, K, 1)) + np.arange(S * K).reshape(S, K, 1)
    P = int(counts.sum()) if max_persons is None else max_persons
    return R.pose_plan_ref(boxes, scores, counts, fn, nf, detect or (0, S), min_score, AR, 1.25, SIZE, posetrack18, P), boxes


# slots (cur, prev, next, pprev, nnext) and margins (left, right, lleft, rright) of the first and the last frame of a video
# of n frames that is wholly in the pool, slot = frame number - first number; written out by hand from the docstring of
# crop.window: nnext is the SAME frame as next, a single neighbour leaves the outer slot on the current frame
ENDS = {
    1: (([0, 0, 0, 0, 0], [0, 0, 0, 0]), ([0, 0, 0, 0, 0], [0, 0, 0, 0])),
    2: (([0, 0, 1, 0, 0], [0, 1, 0, 0]), ([1, 0, 1, 1, 1], [1, 0, 0, 0])),
    3: (([0, 0, 1, 0, 1], [0, 1, 0, 1]), ([2, 1, 2, 0, 2], [1, 0, 2, 0])),
    6: (([0, 0, 1, 0, 1], [0, 1, 0, 1]), ([5, 4, 5, 3, 5], [1, 0, 2, 0])),
}


@pytest.mark.parametrize("posetrack18", [True, False])
@pytest.mark.parametrize("n", sorted(ENDS))
def test_reference_windows_at_both_ends_of_a_video(n, posetrack18):
    fn = list(range(0 if posetrack18 else 1, n + (0 if posetrack18 else 1)))
    ends = sorted({0, n - 1})
    out, _ = _plan(fn, [n] * n, ends, posetrack18)
    assert out["total"] == len(ends)
    for row, (idx, margin) in zip(range(len(ends)), ENDS[n] if n > 1 else ENDS[n][:1]):
        assert out["frame_idx"][row].tolist() == idx and out["margin"][row].tolist() == margin
    assert out["person_slot"].tolist() == ends


def test_reference_two_sequences_back_to_back():
    out, _ = _plan([0, 1, 2, 0, 1, 2, 3], [3, 3, 3, 4, 4, 4, 4], [2, 3, 4])
    assert out["frame_idx"].tolist() == [[2, 1, 2, 0, 2], [3, 3, 4, 3, 4], [4, 3, 5, 4, 5]]
    assert out["margin"].tolist() == [[1, 0, 2, 0], [0, 1, 0, 1], [1, 1, 0, 1]]
    assert out["pr_off"].tolist() == [0, 0, 0, 1, 2, 3, 3, 3]
    # two videos of one length whose numbers restart: still two sequences
    out, _ = _plan([0, 1, 2, 0, 1, 2], [3] * 6, [2, 3])
    assert out["frame_idx"].tolist() == [[2, 1, 2, 0, 2], [3, 3, 4, 3, 4]]


def test_reference_prev_frame_missing_from_the_pool():
    # frames 3, 5, 6 of a 20-frame video: frame 4 (prev of 5) and frames 1, 2, 4 (around 3) are not in the pool
    out, _ = _plan([3, 5, 6], [20] * 3, [0, 1])
    assert out["frame_idx"].tolist() == [[0, 0, 0, -1, -1], [1, 1, 2, 0, 2]]   # prev / next fall back, pprev / nnext become -1
    assert out["margin"].tolist() == [[0, 0, 2, 1], [0, 1, 2, 1]]                # ... and keep their margins (unchecked)


def test_reference_compaction_detect_range_min_score_and_cap():
    scores = [[0.9, 0.2, 0.6], [0.7, 0.7, 0.7], [0.5, 0.1, 0.8], [0.9, 0.9, 0.9]]
    counts = [3, 0, 3, 2]
    out, boxes = _plan([0, 1, 2, 3], [4] * 4, counts, scores=scores, detect=(0, 3), min_score=0.5, max_persons=6)
    assert out["total"] == 4 and out["pr_off"].tolist() == [0, 2, 2, 4, 4]      # slot 3 is halo, slot 1 has count 0
    assert out["person_slot"].tolist() == [0, 0, 2, 2, -1, -1]
    assert out["box_score"][:4].tolist() == [float(np.float32(v)) for v in (0.9, 0.6, 0.5, 0.8)]   # 0.5 itself is kept
    c, s = C.box_to_center_scale(boxes[[0, 0, 2, 2], [0, 2, 0, 2]], AR, 1.25)
    assert np.array_equal(out["center"][:4], c) and np.array_equal(out["scale"][:4], s)
    assert np.array_equal(out["M"][:4], C.crop_matrix(c, s, 0.0, SIZE))
    assert out["M"][4:].tolist() == [[[1, 0, 0], [0, 1, 0]]] * 2 and out["frame_idx"][4:].tolist() == [[-1] * 5] * 2
    assert not out["center"][4:].any() and not out["scale"][4:].any() and not out["margin"][4:].any()
    cut, _ = _plan([0, 1, 2, 3], [4] * 4, counts, scores=scores, detect=(0, 3), min_score=0.5, max_persons=3)
    assert cut["total"] == 4 and cut["pr_off"].tolist() == [0, 2, 2, 3, 3]      # rows truncated, total is not
    assert np.array_equal(cut["center"], out["center"][:3]) and cut["person_slot"].tolist() == [0, 0, 2]


def _random_boxes(n, seed):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(0, 4096, n), rng.uniform(0, 4096, n), rng.uniform(8, 4096, n), rng.uniform(8, 4096, n)], 1)


def test_closed_form_matrix_against_the_lapack_solve():
    """The measurement behind pose_plan_ref.M_MEASURED, repeated: 10^5 boxes, full-size crops; the quirk row (center x -1,
    not enlarged) and the small crops of the GPU test included."""
    boxes = _random_boxes(100000, 0)
    c, s = C.box_to_center_scale(boxes, 288 / 384, 1.25)
    worst = np.abs(closed_form_matrix(c, s, (288, 384)) - C.crop_matrix(c, s, 0.0, (288, 384))).max()
    print("max |closed form - crop_matrix| over 1e5 boxes: %.3e" % worst)
    assert worst <= R.M_TOL
    small = np.array([[-21.0, 5.0, 40.0, 30.0], [3.5, 7.25, 90.0, 20.0], [60.0, 2.0, 11.0, 80.0]])
    c, s = C.box_to_center_scale(small, AR, 1.25)
    assert c[0, 0] == -1 and s[0, 0] == np.float32(40.0 / 200)
    assert np.abs(closed_form_matrix(c, s, SIZE) - C.crop_matrix(c, s, 0.0, SIZE)).max() <= R.M_TOL


# ---- argument errors ------------------------------------------------------------------------------------------------------
def _args(S=3, K=2):
    return [torch.zeros((S, K, 4), dtype=torch.float64), torch.zeros((S, K)), torch.zeros(S, dtype=torch.int32),
            torch.arange(S, dtype=torch.int32), torch.full((S,), S, dtype=torch.int32)]


def test_pose_plan_argument_errors():
    kw = dict(image_size=SIZE, max_persons=8)
    with pytest.raises(NotImplementedError):
        ops.pose_plan(*_args(), **kw)                                           # well-formed, but on the host
    with pytest.raises(ValueError, match="5-frame"):
        ops.pose_plan(*_args(), window_frames=7, **kw)
    for i, dtype in ((0, torch.float32), (1, torch.float64), (2, torch.int64), (3, torch.int64), (4, torch.float32)):
        a = _args()
        a[i] = a[i].to(dtype)
        with pytest.raises(TypeError):
            ops.pose_plan(*a, **kw)
    a = _args()
    a[0] = a[0].numpy()
    with pytest.raises(TypeError):
        ops.pose_plan(*a, **kw)
    for i, shape in ((0, (3, 2, 5)), (0, (3, 8)), (1, (3, 3)), (2, (4,)), (3, (3, 1)), (4, (2,))):
        a = _args()
        a[i] = torch.zeros(shape, dtype=a[i].dtype)
        with pytest.raises(ValueError):
            ops.pose_plan(*a, **kw)
    for bad in (dict(detect=(2, 1)), dict(detect=(0, 4)), dict(detect=(-1, 2)), dict(max_persons=-1), dict(enlarge=0.0),
                dict(aspect_ratio=-1.0), dict(min_score=float("nan")), dict(image_size=(0, 64))):
        with pytest.raises(ValueError):
            ops.pose_plan(*_args(), **{**kw, **bad})


def test_video_pose_argument_errors():
    model = types.SimpleNamespace(cfg=tiny_cfg(8, (64, 96)), training=False, window_frames=5)
    for capacity in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="capacity"):
            VideoPose(model, capacity)
    with pytest.raises(ValueError, match="flip"):
        VideoPose(model, 4, shift_heatmap=True)
    with pytest.raises(ValueError, match="5-frame"):
        VideoPose(types.SimpleNamespace(cfg=model.cfg, training=False, window_frames=7), 4)
    vp = VideoPose(model, 4, flip_test=True, shift_heatmap=True)
    pool = torch.zeros((3, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(TypeError, match="pool"):
        vp.run(pool.float(), *_args())
    with pytest.raises(NotImplementedError):
        vp.run(pool, *_args())                                                  # no CPU path
    with pytest.raises(ValueError, match="max_persons"):
        vp.run(pool, *_args(), max_persons=-1)
    with pytest.raises(ValueError):
        vp.run(pool, *_args(), detect=(2, 1))
    model.training = True
    with pytest.raises(RuntimeError, match="eval"):
        vp.run(pool, *_args())
