"""The training blur fused into the crop (csrc/crop.hip ``otp_crop_clips_blur_u8``): ``ops.crop_clips(blur=...)`` bit for
bit against the numpy restatement in the kernel's order (tests/augment_ref.py), the untouched plain path, and
``OTPose.training_batch`` against the reference's seeded training crops and targets (tests/golden/augment.npz)."""
import os
import random

import numpy as np
import pytest
import torch

from oracle import otpose_oracle as O
from otpose_amd import OTPose, ops, tiny_cfg
from otpose_amd import augment as A
from otpose_amd import crop as C
from otpose_amd import synthetic as S
from otpose_amd import train as TR
from tests import augment_ref as AR
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _pool(s, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (s, h, w, 3)).astype(np.uint8)


def _tables(sigmas):
    return np.stack([[A.blur_table(s) for s in row] for row in np.atleast_2d(sigmas)]).astype(np.float32)


def _check(pool, frame_idx, M, W, H, flip, blur, blur_on=None):
    out = ops.crop_clips(torch.from_numpy(pool).cuda(), frame_idx, M, flip=flip, size=(W, H), blur=blur,
                         blur_on=blur_on)
    ref = O.frames_to_clip(torch.from_numpy(AR.crop_blur_ref(pool, np.asarray(frame_idx), M, W, H, flip, blur,
                                                             blur_on)))
    assert out.shape == ref.shape
    assert torch.equal(out.cpu(), ref)
    return out


# (center, scale) per case on a 37 x 53 frame (Hp x Wp), output 24 x 32 (W x H)
CASES = {
    "inside": ([26.0, 18.0], [0.09, 0.12]),
    "left_edge": ([1.5, 18.0], [0.03, 0.04]),              # reads columns 0..3: the reflection at the left edge
    "right_edge": ([50.7, 20.0], [0.03, 0.04]),            # columns Wp - 4 .. Wp - 1
    "partly_outside": ([2.0, 35.0], [0.12, 0.16]),
    "wholly_outside": ([300.0, -200.0], [0.09, 0.12]),
}


@pytest.mark.parametrize("sigma", [0.1, 5.0])
@pytest.mark.parametrize("rot", [0.0, 17.5, -40.0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_crop_clips_blur_matches_restatement(case, rot, sigma):
    pool = _pool(6, 37, 53, 1)
    c, s = CASES[case]
    B = 3
    M = C.crop_matrix([c] * B, [s] * B, rot, (24, 32))
    frame_idx = np.array([[0, 1, 2, 3, 4], [5, 4, 3, 2, 1], [2, 2, 6, -1, 5]])      # 6 and -1: out of range
    blur = _tables(np.full((B, 5), sigma))
    on = np.array([[1, 1, 1, 1, 1], [1, 0, 1, 0, 1], [0, 1, 1, 1, 0]], np.uint8)
    _check(pool, frame_idx, M, 24, 32, np.array([0, 1, 1], np.uint8), blur, on)
    _check(pool, frame_idx, M, 24, 32, np.array([1, 0, 1], np.uint8), blur)            # blur_on None: all slots


def test_crop_clips_blur_mixed_sigmas_seven_frames_odd_sizes():
    pool = _pool(9, 37, 53, 2)
    M = C.crop_matrix([[10.0, 30.0], [40.0, 5.0]], [[0.2, 0.3], [0.05, 0.07]], [8.0, -95.0], (19, 27))
    frame_idx = torch.tensor([[0, 1, 2, 3, 4, 5, 6], [8, 7, 6, 5, 4, 3, 100]], dtype=torch.int64)
    sig = np.random.RandomState(4).uniform(0.1, 5.0, (2, 7)).astype(np.float32)
    _check(pool, frame_idx, M, 19, 27, [True, False], _tables(sig), sig > 1.0)


def test_crop_clips_blur_narrow_frame():
    pool = _pool(2, 12, 5, 3)                                  # Wp = 5: every tap of the 9 reflects
    M = C.crop_matrix([[2.0, 6.0]], [[0.04, 0.05]], 30.0, (16, 20))
    _check(pool, [[0, 1, 0, 1, 0]], M, 16, 20, [True], _tables([[0.1, 1.0, 2.0, 3.5, 5.0]]))
    with pytest.raises(ValueError):
        ops.crop_clips(torch.from_numpy(_pool(1, 12, 4, 3)).cuda(), [[0] * 5], M, size=(16, 20),
                       blur=_tables([[1.0] * 5]))


@pytest.mark.parametrize("sigma", [0.1, 1.3, 5.0])
def test_identity_crop_is_the_blurred_frame(sigma):
    Hp, Wp = 45, 61
    pool = _pool(2, Hp, Wp, 5)
    M = np.array([[[1.0, 0, 0], [0, 1.0, 0]]])
    t = A.blur_table(sigma)
    for fl in (False, True):
        out = ops.crop_clips(torch.from_numpy(pool).cuda(), [[0, 1, 0, 1, 0]], M, flip=[fl], size=(Wp, Hp),
                             blur=np.broadcast_to(t, (1, 5, 9, 5)).copy())
        src = [p[:, ::-1] if fl else p for p in pool]
        exact = np.stack([AR.blur_frame(src[k], t) for k in (0, 1, 0, 1, 0)])[None]
        assert torch.equal(out.cpu(), O.frames_to_clip(torch.from_numpy(exact)))
        conv = np.stack([AR.blur_frame_conv(src[k], t) for k in (0, 1)])
        d = np.abs(exact[0, :2].astype(np.int16) - conv)
        assert d.max() <= 1 and (d > 0).mean() <= 1e-3


def test_plain_path_unchanged():
    pool = torch.from_numpy(_pool(4, 37, 53, 6)).cuda()
    M = C.crop_matrix([[20.0, 15.0], [30.0, 20.0]], [[0.15, 0.2], [0.2, 0.25]], [0.0, 17.5], (24, 32))
    fi = [[0, 1, 2, 3, 4], [3, 2, 1, 0, -1]]
    plain = ops.crop_clips(pool, fi, M, flip=[0, 1], size=(24, 32))
    assert torch.equal(ops.crop_clips(pool, fi, M, flip=[0, 1], size=(24, 32), blur=None), plain)
    off = ops.crop_clips(pool, fi, M, flip=[0, 1], size=(24, 32), blur=_tables(np.full((2, 5), 2.0)),
                         blur_on=np.zeros((2, 5), np.uint8))
    assert torch.equal(off, plain)
    on = ops.crop_clips(pool, fi, M, flip=[0, 1], size=(24, 32), blur=_tables(np.full((2, 5), 2.0)))
    assert not torch.equal(on, plain)


def _golden_model(g):
    cfg = tiny_cfg(8, tuple(int(v) for v in g["image_size"]))
    cfg.MODEL["SIGMA"] = int(g["sigma_heatmap"][0])
    assert list(cfg.MODEL.HEATMAP_SIZE) == list(g["heatmap_size"])
    return OTPose(cfg).train()


def test_training_batch_matches_reference():
    g = np.load(os.path.join(GOLDEN, "augment.npz"))
    model = _golden_model(g)
    seed = int(g["seed"][0])
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    pool = torch.from_numpy(g["frames"]).cuda()
    x, margin, target, weight = model.training_batch(pool, g["frame_idx"], g["margin"], g["item_joints"],
                                                     g["item_joints_vis"], g["item_center"], g["item_scale"])
    assert torch.equal(target.cpu(), torch.from_numpy(g["target"]))
    assert torch.equal(weight.cpu(), torch.from_numpy(g["target_weight"]))
    assert torch.equal(margin.cpu(), torch.from_numpy(g["margin"]).float())
    ref = O.frames_to_clip(torch.from_numpy(g["crops"]))
    xc = x.cpu()
    blurred = torch.from_numpy(g["sigma"][:, 0] > 0)
    assert torch.equal(xc[~blurred], ref[~blurred])
    lsb = 1.0 / 255 / 0.224 + 1e-5                               # one byte step after Normalize (smallest std)
    d = (xc[blurred] - ref[blurred]).abs()
    assert float(d.max()) <= lsb and float((d > 0).float().mean()) <= 1e-3
    # the same batch from an explicit Augmentation, and bit for bit against the kernel-order restatement
    a = A.Augmentation(g["center"], g["scale"], g["rotation"], g["flip"], g["sigma"], g["joints"], g["joints_vis"])
    x2, _, t2, _ = model.training_batch(pool, g["frame_idx"], g["margin"], g["item_joints"], g["item_joints_vis"],
                                        g["item_center"], g["item_scale"], augment=a)
    assert torch.equal(x2, x) and torch.equal(t2, target)
    W, H = (int(v) for v in g["image_size"])
    M = C.crop_matrix(g["center"], g["scale"], g["rotation"], (W, H))
    tab, on = a.blur_tables()
    exact = AR.crop_blur_ref(g["frames"], g["frame_idx"], M, W, H, g["flip"], tab, on)
    assert torch.equal(xc, O.frames_to_clip(torch.from_numpy(exact)))


def test_crop_clips_blur_cfg2_batch16_every_slot_blurred():
    B, F, W, H = 16, 5, 288, 384
    rng = np.random.RandomState(7)
    pool = rng.randint(0, 256, (20, 720, 1280, 3)).astype(np.uint8)
    boxes = np.stack([rng.uniform(-50, 1200, B), rng.uniform(-50, 650, B), rng.uniform(60, 400, B),
                      rng.uniform(100, 600, B)], axis=1)
    c, s = C.box_to_center_scale(boxes, W / H, 1.25)
    M = C.crop_matrix(c, s, rng.uniform(-45, 45, B), (W, H))
    fi = rng.randint(0, 20, (B, F))
    flip = rng.randint(0, 2, B).astype(np.uint8)
    blur = _tables(rng.uniform(0.1, 5.0, (B, F)))
    out = ops.crop_clips(torch.from_numpy(pool).cuda(), fi, M, flip=flip, size=(W, H), blur=blur).cpu()
    for b in (0, 7):
        ref = AR.crop_blur_ref(pool, fi[b:b + 1], M[b:b + 1], W, H, flip[b:b + 1], blur[b:b + 1])
        assert torch.equal(out[b:b + 1], O.frames_to_clip(torch.from_numpy(ref)))


def test_training_step_on_a_training_batch():
    cfg = tiny_cfg(8, (64, 96))
    model = OTPose(cfg)
    S.fill_synthetic_(model)
    model = model.cuda().train()
    model.train_dropout = False
    rng = np.random.RandomState(9)
    B, Hp, Wp = 3, 120, 160
    pool = torch.from_numpy(rng.randint(0, 256, (6, Hp, Wp, 3)).astype(np.uint8)).cuda()
    boxes = np.array([[30.0, 10.0, 50.0, 90.0], [80.0, 20.0, 60.0, 80.0], [10.0, 40.0, 40.0, 60.0]])
    c, s = C.box_to_center_scale(boxes, 64 / 96, 1.25)
    joints = np.zeros((B, 17, 3))
    joints[..., 0] = boxes[:, None, 0] + rng.uniform(0, 1, (B, 17)) * boxes[:, None, 2]
    joints[..., 1] = boxes[:, None, 1] + rng.uniform(0, 1, (B, 17)) * boxes[:, None, 3]
    vis = np.ones((B, 17, 3))
    vis[..., 2] = 0
    idx, margin = zip(*[C.window(k, 6) for k in (0, 3, 5)])
    torch.manual_seed(1)
    np.random.seed(1)
    random.seed(1)
    x, m, target, weight = model.training_batch(pool, np.array(idx), np.array(margin), joints, vis, c, s)
    assert x.shape == (B, 15, 96, 64) and target.shape == (B, 17, 24, 16) and weight.shape == (B, 17, 1)
    outs = TR.forward_train(model, x, m)
    loss = TR.criterion(outs, target, weight)
    loss.backward()
    assert bool(torch.isfinite(loss))
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())
