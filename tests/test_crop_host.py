"""Host side of the video -> crop step (otpose_amd/crop.py) against the reference-generated tests/golden/crop.npz, the
window rule's known answers, the numpy restatement of csrc/crop.hip (tests/crop_ref.py) on known answers, and the
argument checks of the two C entry points.  No GPU needed."""
import os

import numpy as np
import pytest

from otpose_amd import crop as C
from otpose_amd import hip
from tests import crop_ref as R
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "crop.npz"))


def test_box_to_center_scale_matches_reference(g):
    for k, enl in enumerate(g["box_enlarge"]):
        c, s = C.box_to_center_scale(g["boxes"], g["aspect"][0], enl)
        assert c.dtype == np.float32 and s.dtype == np.float32
        assert np.array_equal(c, g[f"box_center_{k}"]) and np.array_equal(s, g[f"box_scale_{k}"])


def test_crop_matrix_matches_reference(g):
    c, s = g["box_center_1"], g["box_scale_1"]
    for i, r in enumerate(g["rots"]):
        for inv in (0, 1):
            M = C.crop_matrix(c, s, r, (288, 384), inv=bool(inv))
            assert M.shape == (len(c), 2, 3) and M.dtype == np.float64
            assert np.array_equal(M, g["trans"][i, inv]), (r, inv)
    # per-sample rotations in one call
    n = len(c)
    M = C.crop_matrix(np.repeat(c, 3, 0), np.repeat(s, 3, 0), np.tile(g["rots"], n), (288, 384))
    assert np.array_equal(M.reshape(n, 3, 2, 3).transpose(1, 0, 2, 3), g["trans"][:, 0])


def test_point_transform_matches_reference_to_the_last_bits(g):
    """exec_affine_transform: the kernel's plain left-to-right sums vs numpy's dot (BLAS order) - equal up to rounding."""
    moved = R.affine_points(g["trans"][1, 0], g["pts"])
    assert np.allclose(moved, g["pts_moved"], rtol=1e-13, atol=1e-9)


@pytest.mark.parametrize("sigma", [2, 3])
def test_target_restatement_matches_reference(g, sigma):
    """Visibility cut + generate_heatmaps of the restatement (identity crop matrix) == the reference, bit for bit."""
    joints, vis = g["joints"][..., :2], g["joints_vis"][..., 0].astype(np.float32)
    eye = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (len(joints), 1, 1))
    t, w = R.pose_targets_ref(joints, vis, eye, sigma, (288, 384), (72, 96))
    assert np.array_equal(t, g[f"target_s{sigma}"]) and np.array_equal(w, g[f"target_weight_s{sigma}"])


def test_gaussian_table():
    t = C.gaussian_table(2)
    assert t.shape == (13, 13) and t.dtype == np.float32 and t[6, 6] == 1.0 and np.array_equal(t, t.T)
    with pytest.raises(ValueError):
        C.gaussian_table(2.5)


@pytest.mark.parametrize("pt18, cur, n, frames, margin", [
    # PoseTrack18: frames numbered from 0
    (True, 0, 10, [0, 0, 1, 0, 1], [0, 1, 0, 1]),
    (True, 1, 10, [1, 0, 2, 1, 2], [1, 1, 0, 1]),
    (True, 5, 10, [5, 4, 6, 3, 6], [1, 1, 2, 1]),       # nnext == next (the reference takes next_delta_range[0])
    (True, 8, 10, [8, 7, 9, 6, 8], [1, 1, 2, 0]),
    (True, 9, 10, [9, 8, 9, 7, 9], [1, 0, 2, 0]),
    # PoseTrack17: frames numbered from 1
    (False, 1, 10, [1, 1, 2, 1, 2], [0, 1, 0, 1]),
    (False, 2, 10, [2, 1, 3, 2, 3], [1, 1, 0, 1]),
    (False, 9, 10, [9, 8, 10, 7, 9], [1, 1, 2, 0]),
    (False, 10, 10, [10, 9, 10, 8, 10], [1, 0, 2, 0]),
    # one-, two- and three-frame videos
    (True, 0, 1, [0, 0, 0, 0, 0], [0, 0, 0, 0]),
    (False, 1, 1, [1, 1, 1, 1, 1], [0, 0, 0, 0]),
    (True, 0, 2, [0, 0, 1, 0, 0], [0, 1, 0, 0]),
    (True, 1, 2, [1, 0, 1, 1, 1], [1, 0, 0, 0]),
    (False, 2, 2, [2, 1, 2, 2, 2], [1, 0, 0, 0]),
    (True, 0, 3, [0, 0, 1, 0, 1], [0, 1, 0, 1]),
    (True, 1, 3, [1, 0, 2, 1, 1], [1, 1, 0, 0]),
    (True, 2, 3, [2, 1, 2, 0, 2], [1, 0, 2, 0]),
])
def test_window_known_answers(pt18, cur, n, frames, margin):
    assert C.window(cur, n, posetrack18=pt18) == (frames, margin)


def test_window_missing_frame_falls_back_to_current():
    assert C.window(5, 10, available={3, 5, 6}) == ([5, 5, 6, 3, 6], [0, 1, 2, 1])
    assert C.window(5, 10, available=lambda k: k != 6) == ([5, 4, 5, 3, 6], [1, 0, 2, 1])


def _frame(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def test_restatement_identity_is_an_exact_copy():
    src = _frame(37, 53, 1)
    eye = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    assert np.array_equal(R.warp_affine(src, eye, 53, 37), src)
    big = R.warp_affine(src, eye, 60, 40)
    assert np.array_equal(big[:37, :53], src) and not big[37:].any() and not big[:, 53:].any()


def test_restatement_integer_translation_is_a_shifted_copy():
    src = _frame(37, 53, 2)
    M = np.array([[1.0, 0, -7], [0, 1.0, 5]])          # crop(x, y) = src(x + 7, y - 5)
    out = R.warp_affine(src, M, 53, 37)
    assert np.array_equal(out[5:, :46], src[:32, 7:])
    assert not out[:5].any() and not out[:, 46:].any()


def test_restatement_2x_zoom_gives_fixed_point_averages():
    src = _frame(20, 30, 3).astype(np.int64)
    out = R.warp_affine(src.astype(np.uint8), np.array([[2.0, 0, 0], [0, 2.0, 0]]), 58, 38).astype(np.int64)
    assert np.array_equal(out[0::2, 0::2], src[:19, :29])
    assert np.array_equal(out[0::2, 1::2], (src[:19, :29] + src[:19, 1:30] + 1) >> 1)
    assert np.array_equal(out[1::2, 0::2], (src[:19, :29] + src[1:20, :29] + 1) >> 1)
    quad = src[:19, :29] + src[:19, 1:30] + src[1:20, :29] + src[1:20, 1:30]
    assert np.array_equal(out[1::2, 1::2], (quad + 2) >> 2)


def test_restatement_flip_is_the_warp_of_the_mirrored_frame():
    src = _frame(37, 53, 4)
    M = C.crop_matrix([[20.3, 17.9]], [[0.11, 0.15]], 17.5, (24, 32))[0]
    assert np.array_equal(R.warp_affine(src, M, 24, 32, flip=True), R.warp_affine(src[:, ::-1], M, 24, 32))


def test_crop_symbols_reject_bad_arguments_without_a_gpu():
    L = hip.lib()
    m = [0.485, 0.456, 0.406]
    s = [0.229, 0.224, 0.225]
    assert L.otp_crop_clips_u8(None, 1, 8, 8, None, None, None, None, 1, 5, 4, 4, *m, *s, None) == -1
    assert L.otp_crop_clips_u8(1, 0, 8, 8, 1, 1, None, 1, 1, 5, 4, 4, *m, *s, None) == -1            # S = 0
    assert L.otp_crop_clips_u8(1, 1, 8, 8, 1, 1, None, 1, 1, 5, 0, 4, *m, *s, None) == -1            # H = 0
    assert L.otp_crop_clips_u8(1, 1, 8, 40000, 1, 1, None, 1, 1, 5, 4, 4, *m, *s, None) == -2        # Wp > 32767
    assert L.otp_crop_clips_u8(1, 1, 8, 8, 1, 1, None, 1, 1, 5, 4, 4, *m, 0.229, 0.0, 0.225, None) == -2
    assert L.otp_pose_targets(None, None, None, None, None, None, 1, 17, 288, 384, 72, 96, 6, None) == -1
    assert L.otp_pose_targets(1, 1, 1, 1, 1, 1, 1, 0, 288, 384, 72, 96, 6, None) == -1                # J = 0
