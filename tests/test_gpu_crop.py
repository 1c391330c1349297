"""Person crops from whole frames on the GPU (csrc/crop.hip): ``ops.crop_clips`` bit for bit against the numpy
restatement of cv2.warpAffine (tests/crop_ref.py) + the oracle's ToTensor / Normalize, ``OTPose.forward_video`` /
``predict`` against the forward of the same crops, and ``ops.pose_targets`` against the reference's targets."""
import os

import numpy as np
import pytest
import torch

from oracle import otpose_oracle as O
from otpose_amd import OTPose, ops, tiny_cfg
from otpose_amd import crop as C
from otpose_amd import synthetic as S
from tests import crop_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _pool(s, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (s, h, w, 3)).astype(np.uint8)


def _check(pool, frame_idx, M, W, H, flip=None):
    out = ops.crop_clips(torch.from_numpy(pool).cuda(), frame_idx, M, flip=flip, size=(W, H))
    ref = O.frames_to_clip(torch.from_numpy(R.crop_ref(pool, np.asarray(frame_idx), M, W, H, flip)))
    assert out.shape == ref.shape
    assert torch.equal(out.cpu(), ref)
    return out


# (center, scale) per case on a 37 x 53 frame (Hp x Wp), output 24 x 32 (W x H)
CASES = {
    "inside": ([26.0, 18.0], [0.09, 0.12]),
    "partly_outside": ([2.0, 35.0], [0.12, 0.16]),
    "wholly_outside": ([300.0, -200.0], [0.09, 0.12]),
    "zoom_x8": ([20.5, 11.3], [24 / 200 / 8, 32 / 200 / 8]),
    "zoom_x0.1": ([26.0, 18.0], [24 / 200 / 0.1, 32 / 200 / 0.1]),
}


@pytest.mark.parametrize("rot", [0.0, 17.5, -40.0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_crop_clips_small_pool(case, rot):
    pool = _pool(6, 37, 53, 1)
    c, s = CASES[case]
    B = 3
    M = C.crop_matrix([c] * B, [s] * B, rot, (24, 32))
    frame_idx = np.array([[0, 1, 2, 3, 4], [5, 4, 3, 2, 1], [2, 2, 6, -1, 5]])      # 6 and -1: out of range
    _check(pool, frame_idx, M, 24, 32, flip=np.array([0, 1, 1], np.uint8))


def test_crop_clips_seven_frames_and_odd_sizes():
    pool = _pool(9, 37, 53, 2)
    M = C.crop_matrix([[10.0, 30.0], [40.0, 5.0]], [[0.2, 0.3], [0.05, 0.07]], [8.0, -95.0], (19, 27))
    frame_idx = torch.tensor([[0, 1, 2, 3, 4, 5, 6], [8, 7, 6, 5, 4, 3, 100]], dtype=torch.int64)
    _check(pool, frame_idx, M, 19, 27, flip=[True, False])


def test_crop_clips_720p_pool():
    pool = _pool(4, 720, 1280, 3)
    c, s = C.box_to_center_scale([[600.3, 200.7, 180.0, 400.0], [1200.0, 650.0, 300.0, 300.0]], 288 / 384, 1.25)
    M = C.crop_matrix(c, s, [0.0, 17.5], (288, 384))
    _check(pool, [[0, 1, 2, 3, 0], [3, 2, 1, 0, 3]], M, 288, 384, flip=[False, True])


def test_crop_clips_mixed_size_padded_pool_equals_per_size_calls():
    small, big = _pool(2, 30, 40, 4), _pool(2, 37, 53, 5)
    padded = np.zeros((4, 37, 53, 3), np.uint8)
    padded[:2, :30, :40] = small
    padded[2:] = big
    M = C.crop_matrix([[20.0, 15.0], [30.0, 20.0]], [[0.15, 0.2], [0.2, 0.25]], [0.0, 17.5], (24, 32))
    mixed = ops.crop_clips(torch.from_numpy(padded).cuda(), [[0, 1, 0, 1, 0], [2, 3, 2, 3, 2]], M, size=(24, 32))
    a = ops.crop_clips(torch.from_numpy(small).cuda(), [[0, 1, 0, 1, 0]], M[:1], size=(24, 32))
    b = ops.crop_clips(torch.from_numpy(big).cuda(), [[0, 1, 0, 1, 0]], M[1:], size=(24, 32))
    assert torch.equal(mixed[:1], a) and torch.equal(mixed[1:], b)
    assert torch.equal(a.cpu(), O.frames_to_clip(torch.from_numpy(R.crop_ref(small, [[0, 1, 0, 1, 0]], M[:1], 24, 32))))


def test_crop_clips_cfg2_batch16_shape():
    """The full cfg2 input: 16 persons x 5 frames of 384 x 288 from a 20-frame 720p pool."""
    pool = _pool(20, 720, 1280, 6)
    rng = np.random.RandomState(7)
    boxes = np.stack([rng.uniform(-50, 1200, 16), rng.uniform(-50, 650, 16), rng.uniform(40, 500, 16),
                      rng.uniform(60, 700, 16)], axis=1)
    c, s = C.box_to_center_scale(boxes, 288 / 384, 1.25)
    M = C.crop_matrix(c, s, rng.uniform(-45, 45, 16), (288, 384))
    frame_idx = rng.randint(0, 20, (16, 5))
    out = _check(pool, frame_idx, M, 288, 384, flip=rng.randint(0, 2, 16).astype(np.uint8))
    assert out.shape == (16, 15, 384, 288)


def test_crop_clips_checks_inputs():
    pool = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    M = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (1, 1, 1))
    with pytest.raises(TypeError):
        ops.crop_clips(pool.float(), [[0] * 5], M, size=(4, 4))
    with pytest.raises(ValueError):
        ops.crop_clips(pool, [[0] * 5], M[:, :1], size=(4, 4))
    with pytest.raises(ValueError):
        ops.crop_clips(pool, np.array([[0, 1, 2 ** 33, 0, 0]]), M, size=(4, 4))
    with pytest.raises(ValueError):
        ops.crop_clips(pool, [[0] * 5], M)                      # no size
    with pytest.raises(NotImplementedError):
        ops.crop_clips(pool.cpu(), [[0] * 5], M, size=(4, 4))


# ---- the model on whole frames ----------------------------------------------------------------------------------------
def _video_inputs(cfg, B=2, seed=8):
    w_img, h_img = cfg.MODEL.IMAGE_SIZE
    pool = _pool(7, 90, 130, seed)
    c, s = C.box_to_center_scale([[30.0, 10.0, 40.0, 60.0], [70.5, 40.2, 50.0, 45.0]][:B], w_img / h_img, 1.25)
    frames, margins = zip(*[C.window(k, 7) for k in (0, 4)][:B])
    return pool, np.array(frames), c, s, torch.tensor(margins, dtype=torch.float32)


def _model(cfg):
    m = OTPose(cfg)
    S.fill_synthetic_(m)
    return m.cuda()


@pytest.mark.parametrize("width, size, dtype", [(8, (64, 96), "fp32"), (16, (128, 192), "fp16")])
def test_forward_video_equals_forward_frames_of_reference_crops(width, size, dtype):
    cfg = tiny_cfg(width, size, dtype=dtype)
    model = _model(cfg).eval()
    pool, fi, c, s, margin = _video_inputs(cfg)
    M = C.crop_matrix(c, s, 0.0, size)
    crops = torch.from_numpy(R.crop_ref(pool, fi, M, *size))
    with torch.no_grad():
        a = [t.clone() for t in model.forward_video(torch.from_numpy(pool).cuda(), fi, c, s, margin)]
        engine, inp = model._engine, model._engine.inp.data_ptr()
        a2 = model.forward_video(torch.from_numpy(pool).cuda(), fi, c, s, margin.cuda())
        assert model._engine is engine and model._engine.inp.data_ptr() == inp      # same engine, same input buffer
        b = model.forward_frames(crops.cuda(), margin.cuda())
    for u, u2, v in zip(a, a2, b):
        assert torch.equal(u, v) and torch.equal(u2, v)


def test_forward_video_train_mode_equals_forward_of_the_same_clip():
    cfg = tiny_cfg(8, (64, 96))
    model = _model(cfg).train()
    model.train_dropout = False
    pool, fi, c, s, margin = _video_inputs(cfg)
    rot, flip = np.array([10.0, -20.0]), np.array([1, 0], np.uint8)
    M = C.crop_matrix(c, s, rot, (64, 96))
    clip = O.frames_to_clip(torch.from_numpy(R.crop_ref(pool, fi, M, 64, 96, flip))).cuda()
    torch.manual_seed(5)
    a = model.forward_video(torch.from_numpy(pool).cuda(), fi, c, s, margin, rotation=rot, flip=flip)
    torch.manual_seed(5)
    b = model(clip, margin=margin.cuda())
    for u, v in zip(a, b):
        assert torch.equal(u.detach(), v.detach())


def test_predict_equals_get_final_preds_of_the_output():
    cfg = tiny_cfg(8, (64, 96))
    model = _model(cfg).eval()
    pool, fi, c, s, margin = _video_inputs(cfg)
    with torch.no_grad():
        preds, maxvals = model.predict(torch.from_numpy(pool).cuda(), fi, c, s, margin)
        out = model.forward_video(torch.from_numpy(pool).cuda(), fi, c, s, margin)
        p2, m2 = ops.get_final_preds(out[0], torch.from_numpy(c), torch.from_numpy(s))
    assert preds.shape == (2, cfg.MODEL.NUM_JOINTS, 2)
    assert torch.equal(preds, p2) and torch.equal(maxvals, m2)


# ---- training targets -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [2, 3])
def test_pose_targets_match_reference(sigma):
    g = np.load(os.path.join(GOLDEN, "crop.npz"))
    joints, vis = g["joints"], g["joints_vis"]
    eye = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (len(joints), 1, 1))
    t, w = ops.pose_targets(torch.from_numpy(joints).cuda(), vis, eye, sigma, (288, 384), (72, 96))
    assert torch.equal(t.cpu(), torch.from_numpy(g[f"target_s{sigma}"]))
    assert torch.equal(w.cpu(), torch.from_numpy(g[f"target_weight_s{sigma}"]))


def test_pose_targets_batch16_match_restatement():
    rng = np.random.RandomState(9)
    B, J = 16, 17
    boxes = np.stack([rng.uniform(0, 1000, B), rng.uniform(0, 500, B), rng.uniform(50, 300, B),
                      rng.uniform(80, 400, B)], axis=1)
    c, s = C.box_to_center_scale(boxes, 288 / 384, 1.25)
    M = C.crop_matrix(c, s, rng.uniform(-40, 40, B), (288, 384))
    joints = boxes[:, None, :2] + rng.uniform(-0.3, 1.3, (B, J, 2)) * boxes[:, None, 2:]
    vis = (rng.uniform(0, 1, (B, J)) > 0.2).astype(np.float32)
    for sigma in (2, 3):
        t, w = ops.pose_targets(joints, vis, torch.from_numpy(M).cuda(), sigma, (288, 384), (72, 96))
        rt, rw = R.pose_targets_ref(joints, vis, M, sigma, (288, 384), (72, 96))
        assert torch.equal(t.cpu(), torch.from_numpy(rt)) and torch.equal(w.cpu(), torch.from_numpy(rw))
        assert 0 < float(rw.sum()) < B * J
