"""Training augmentation on the host (otpose_amd/augment.py) against the reference-generated tests/golden/augment.npz,
and the numpy restatement of the fused blur + warp (tests/augment_ref.py) against the reference's crops.  No GPU needed."""
import os
import random

import numpy as np
import pytest
import torch

from otpose_amd import augment as A
from otpose_amd import hip
from tests import augment_ref as AR
from tests import crop_ref as R
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "augment.npz"))


def _sample(g, global_rngs=True, **kw):
    s = int(g["seed"][0])
    if global_rngs:
        np.random.seed(s)
        random.seed(s)
        torch.manual_seed(s)
        rngs = {}
    else:
        rngs = dict(np_rng=np.random.RandomState(s), py_rng=random.Random(s), torch_gen=torch.Generator().manual_seed(s))
    w, h = g["image_size"]
    return A.sample_augmentation(g["item_joints"], g["item_joints_vis"], g["item_center"], g["item_scale"],
                                 g["frames"].shape[2], scale_factor=[0.35, 0.35], rotation_factor=45, flip=True,
                                 prob_half_body=0.3, num_joints_half_body=8, aspect_ratio=w * 1.0 / h, **rngs, **kw)


@pytest.mark.parametrize("global_rngs", [True, False])
def test_sample_augmentation_reproduces_the_seeded_reference(g, global_rngs):
    a = _sample(g, global_rngs)
    for name, key in (("center", "center"), ("scale", "scale"), ("rotation", "rotation"), ("flip", "flip"),
                      ("blur_sigma", "sigma"), ("joints", "joints"), ("joints_vis", "joints_vis")):
        got = getattr(a, name)
        assert got.dtype == g[key].dtype, name
        assert np.array_equal(got, g[key]), name
    assert a.center.dtype == np.float32 and a.scale.dtype == np.float32 and a.rotation.dtype == np.float64


def test_golden_covers_every_branch(g, monkeypatch):
    taken = []
    orig = A.half_body

    def rec(joints, vis, aspect_ratio, rng):
        c, s = orig(joints, vis, aspect_ratio, rng)
        up = np.array([joints[k] for k in A.UPPER_BODY_IDS if vis[k][0] > 0], np.float32).mean(axis=0)[:2]
        taken.append("upper" if np.array_equal(c, up) else "lower")
        return c, s

    monkeypatch.setattr(A, "half_body", rec)
    _sample(g)
    assert {"upper", "lower"} <= set(taken)
    for mask in (g["flip"], g["rotation"] != 0, g["sigma"][:, 0] > 0):
        assert mask.any() and not mask.all()
    assert (g["frame_idx"][:, 0] == 0).any() and (g["frame_idx"][:, 0] == g["frames"].shape[0] - 1).any()
    assert (g["item_joints_vis"][..., 0] == 0).any()


def test_fliplr_joints_matches_reference(g):
    for b in np.nonzero(g["flip"])[0]:
        j, v = A.fliplr_joints(g["item_joints"][b], g["item_joints_vis"][b], g["frames"].shape[2])
        assert np.array_equal(j, g["joints"][b]) and np.array_equal(v, g["joints_vis"][b])
    j, v = A.fliplr_joints(np.arange(51.0).reshape(17, 3), np.ones((17, 3)), 100)
    assert j[0, 0] == 99.0 and j[3, 0] == 100 - 12 - 1 and j[4, 0] == 100 - 9 - 1
    vis = np.ones((17, 3))
    vis[4] = 0
    j, v = A.fliplr_joints(np.ones((17, 3)) * 5, vis, 100)
    assert not j[3].any() and v[3, 0] == 0 and v[4, 0] == 1               # swapped, then zeroed by joints * vis


def test_half_body_known_answers():
    joints = np.zeros((17, 3))
    joints[:, 0] = np.arange(17) * 2.0
    joints[:, 1] = np.arange(17) * 3.0 + 1
    vis = np.ones((17, 3))

    class Fixed:
        def __init__(self, v):
            self.v = v

        def randn(self):
            return self.v

    c, s = A.half_body(joints, vis, 0.75, Fixed(0.0))               # < 0.5: upper body (ids 0..10)
    assert c.dtype == np.float32 and s.dtype == np.float32
    assert np.array_equal(c, np.array([10.0, 16.0], np.float32))
    h = 30.0
    assert np.array_equal(s, np.array([h * 0.75 / 200, h / 200], np.float32) * 1.5)
    c, _ = A.half_body(joints, vis, 0.75, Fixed(0.7))               # lower body (ids 11..16)
    assert np.array_equal(c, np.array([27.0, 41.5], np.float32))
    one = np.zeros((17, 3))
    one[0] = 1
    assert A.half_body(joints, one, 0.75, Fixed(0.0)) == (None, None)      # unreachable behind the dataset's guard


def test_blur_table_is_torchvision_kernel(g):
    t = A.blur_table(1.5)
    assert t.shape == (9, 5) and t.dtype == np.float32
    assert abs(float(t.astype(np.float64).sum()) - 1.0) < 1e-6
    assert np.array_equal(t, t[::-1]) and np.array_equal(t, t[:, ::-1])
    assert t[4, 2] == t.max()
    # the reference's crops are the warps of conv2d-blurred frames: blur_table reproduces them bit for bit
    frames, W, H = g["frames"], int(g["image_size"][0]), int(g["image_size"][1])
    for b in np.nonzero(g["sigma"][:, 0] > 0)[0][:4]:
        M = _matrix(g, b)
        for f in range(5):
            src = frames[g["frame_idx"][b, f]]
            src = src[:, ::-1] if g["flip"][b] else src
            blurred = AR.blur_frame_conv(src, A.blur_table(g["sigma"][b, f]))
            assert np.array_equal(R.warp_affine(blurred, M, W, H), g["crops"][b, f])


def _matrix(g, b):
    from otpose_amd import crop as C
    return C.crop_matrix(g["center"][b:b + 1], g["scale"][b:b + 1], g["rotation"][b], tuple(g["image_size"]))[0]


def test_kernel_order_restatement_against_reference_crops(g):
    from otpose_amd import crop as C
    W, H = int(g["image_size"][0]), int(g["image_size"][1])
    M = C.crop_matrix(g["center"], g["scale"], g["rotation"], (W, H))
    tab = np.stack([[A.blur_table(s) if s > 0 else np.zeros((9, 5), np.float32) for s in row] for row in g["sigma"]])
    out = AR.crop_blur_ref(g["frames"], g["frame_idx"], M, W, H, g["flip"], tab, g["sigma"] > 0)
    blurred = g["sigma"][:, 0] > 0
    assert np.array_equal(out[~blurred], g["crops"][~blurred])
    d = np.abs(out[blurred].astype(np.int16) - g["crops"][blurred].astype(np.int16))
    assert d.max() <= 1 and (d > 0).mean() <= 1e-3


def test_kernel_order_blur_against_conv2d_on_a_noisy_frame():
    f = np.random.RandomState(3).randint(0, 256, (40, 90, 3)).astype(np.uint8)
    for s in (0.1, 0.7, 2.5, 5.0):
        t = A.blur_table(s)
        a, c = AR.blur_frame(f, t), AR.blur_frame_conv(f, t)
        d = np.abs(a.astype(np.int16) - c)
        assert d.max() <= 1 and (d > 0).mean() <= 1e-3
    assert np.array_equal(AR.blur_frame(f, A.blur_table(0.1)), f)       # sigma 0.1: the centre tap is 1.0


def test_blur_tables_and_sigma_draws(g):
    a = _sample(g)
    tab, on = a.blur_tables()
    assert tab.shape == (24, 5, 9, 5) and on.dtype == np.uint8
    assert np.array_equal(on.astype(bool), a.blur_sigma > 0)
    assert ((a.blur_sigma == 0) | ((a.blur_sigma >= 0.1) & (a.blur_sigma <= 5))).all()
    b, f = np.argwhere(on)[0]
    assert np.array_equal(tab[b, f], A.blur_table(a.blur_sigma[b, f]))


def test_blur_symbol_rejects_bad_arguments_without_a_gpu():
    L = hip.lib()
    m = [0.485, 0.456, 0.406]
    s = [0.229, 0.224, 0.225]
    assert L.otp_crop_clips_blur_u8(1, 1, 8, 8, 1, 1, None, 1, 1, 5, 4, 4, *m, *s, None, None, None) == -1   # blur NULL
    assert L.otp_crop_clips_blur_u8(None, 1, 8, 8, 1, 1, None, 1, 1, 5, 4, 4, *m, *s, 1, None, None) == -1
    assert L.otp_crop_clips_blur_u8(1, 1, 8, 4, 1, 1, None, 1, 1, 5, 4, 4, *m, *s, 1, None, None) == -2      # Wp < 5
    assert L.otp_crop_clips_blur_u8(1, 1, 8, 40000, 1, 1, None, 1, 1, 5, 4, 4, *m, *s, 1, None, None) == -2
