"""Flip test on the GPU: the mirrored twin crops (``ops.crop_clips(mirror_pair=True)``), ``ops.mirror_pair`` and the fused
flip-back decode (``ops.flip_test_merge``) bit for bit against torch / the numpy restatement (tests/flip_ref.py), and
``OTPose.predict(flip_test=True)`` / ``flip_test_heatmaps`` against the same engine's forward and the oracle."""
import numpy as np
import pytest
import torch

from oracle import otpose_oracle as O
from otpose_amd import OTPose, augment, ops, tiny_cfg
from otpose_amd import crop as C
from otpose_amd import synthetic as S
from tests import flip_ref as R

pytestmark = pytest.mark.gpu
PERM = ops.flip_permutation(augment.FLIP_PAIRS, 17)


def _pool(s, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (s, h, w, 3)).astype(np.uint8)


def _check_pair(pool, frame_idx, M, W, H):
    pool = torch.from_numpy(pool).cuda()
    pair = ops.crop_clips(pool, frame_idx, M, size=(W, H), mirror_pair=True)
    plain = ops.crop_clips(pool, frame_idx, M, size=(W, H))
    b = plain.shape[0]
    assert pair.shape == (2 * b,) + tuple(plain.shape[1:])
    assert torch.equal(pair[:b], plain)
    assert torch.equal(pair[b:], torch.flip(plain, [3]))
    out = torch.full_like(pair, float("nan"))
    assert ops.crop_clips(pool, frame_idx, M, out=out, mirror_pair=True) is out
    assert torch.equal(out, pair)
    return pair


@pytest.mark.parametrize("W, H", [(24, 32), (19, 27), (1, 5)])
def test_pair_crop_small_pools_and_odd_widths(W, H):
    pool = _pool(6, 37, 53, 1)
    M = C.crop_matrix([[26.0, 18.0], [2.0, 35.0], [300.0, -200.0]], [[0.09, 0.12], [0.12, 0.16], [0.09, 0.12]],
                      [0.0, 17.5, -40.0], (W, H))
    _check_pair(pool, [[0, 1, 2, 3, 4], [5, 4, 3, 2, 1], [2, 2, 6, -1, 5]], M, W, H)


def test_pair_crop_seven_frames():
    pool = _pool(9, 37, 53, 2)
    M = C.crop_matrix([[10.0, 30.0], [40.0, 5.0]], [[0.2, 0.3], [0.05, 0.07]], [8.0, -95.0], (19, 27))
    _check_pair(pool, [[0, 1, 2, 3, 4, 5, 6], [8, 7, 6, 5, 4, 3, 100]], M, 19, 27)


def test_pair_crop_cfg2_batch16_shape():
    pool = _pool(20, 720, 1280, 6)
    rng = np.random.RandomState(7)
    boxes = np.stack([rng.uniform(-50, 1200, 16), rng.uniform(-50, 650, 16), rng.uniform(40, 500, 16),
                      rng.uniform(60, 700, 16)], axis=1)
    c, s = C.box_to_center_scale(boxes, 288 / 384, 1.25)
    M = C.crop_matrix(c, s, 0.0, (288, 384))
    pair = _check_pair(pool, rng.randint(0, 20, (16, 5)), M, 288, 384)
    assert pair.shape == (32, 15, 384, 288)


def test_pair_crop_checks_inputs():
    pool = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    M = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (1, 1, 1))
    with pytest.raises(ValueError):
        ops.crop_clips(pool, [[0] * 5], M, flip=[True], size=(4, 4), mirror_pair=True)
    with pytest.raises(ValueError):
        ops.crop_clips(pool, [[0] * 5], M, blur=np.zeros((1, 5, 9, 5), np.float32), size=(4, 4), mirror_pair=True)
    with pytest.raises(ValueError):                             # a (B, ...) out for a (2B, ...) result
        ops.crop_clips(pool, [[0] * 5], M, out=torch.empty((1, 15, 4, 4), device="cuda"), mirror_pair=True)


@pytest.mark.parametrize("shape", [(2, 15, 384, 288), (3, 15, 7, 9), (1, 21, 5, 1), (2, 6, 3, 8)])
def test_mirror_pair_equals_cat_of_x_and_its_flip(shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape))).cuda()
    want = torch.cat([x, x.flip(3)])
    assert torch.equal(ops.mirror_pair(x), want)
    out = torch.full_like(want, float("nan"))
    assert ops.mirror_pair(x, out=out) is out and torch.equal(out, want)


def test_mirror_pair_unaligned_views():
    base = torch.randn(2 * 3 * 4 * 8 + 1, device="cuda")
    x = base[1:].view(2, 3, 4, 8)                               # 4-byte offset: the one-float-per-thread form
    assert torch.equal(ops.mirror_pair(x), torch.cat([x, x.flip(3)]))


def _maps(b, j, h, w, seed):
    return np.random.RandomState(seed).standard_normal((2 * b, j, h, w)).astype(np.float32)


def _merge_and_compare(hm, shift, pairs=augment.FLIP_PAIRS):
    j = hm.shape[1]
    merged, preds, maxvals = ops.flip_test_merge(torch.from_numpy(hm).cuda(), pairs, shift_heatmap=shift)
    want = R.flip_merge(hm, ops.flip_permutation(pairs, j), shift)
    assert np.array_equal(merged.cpu().numpy(), want, equal_nan=True)
    rp, rm = R.final_preds(want)
    assert np.array_equal(preds.cpu().numpy(), rp) and np.array_equal(maxvals.cpu().numpy(), rm, equal_nan=True)
    p2, m2 = ops.get_final_preds(merged)
    assert torch.equal(preds, p2) and np.array_equal(maxvals.cpu().numpy(), m2.cpu().numpy(), equal_nan=True)
    return merged, preds, maxvals


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("b, h, w", [(1, 96, 72), (16, 96, 72), (2, 9, 13), (3, 5, 1)])
def test_flip_test_merge_equals_restatement(b, h, w, shift):
    _merge_and_compare(_maps(b, 17, h, w, b * h + w + shift), shift)


@pytest.mark.parametrize("shift", [False, True])
def test_flip_test_merge_ties_nans_and_negative_planes(shift):
    b, j, h, w = 3, 17, 12, 11
    hm = _maps(b, j, h, w, 5)
    hm[0, 3] = 0.25                                             # a flat plane: ties everywhere, first maximum wins
    hm[b + 0, 4] = 0.25
    hm[1, 5, 4, 6] = hm[1, 5, 7, 2] = 50.0                      # two planted maxima in the plain half
    hm[b + 1, 6] = 0.0
    hm[b + 2, 8, 2, 3] = np.nan                                 # a NaN in the mirrored half (lands in plane 7 of sample 2)
    hm[2, 0, 6, 6] = np.nan                                     # and in the plain half, next to a later one
    hm[2, 0, 9, 1] = np.nan
    hm[1, 9] = -np.abs(hm[1, 9]) - 1.0                          # all-negative merged plane: the maxvals > 0 mask
    hm[b + 1, 10] = -np.abs(hm[b + 1, 10]) - 1.0
    merged, preds, maxvals = _merge_and_compare(hm, shift)
    assert torch.isnan(maxvals[2, 7, 0]) and torch.isnan(maxvals[2, 0, 0])
    assert torch.equal(preds[1, 9], torch.zeros(2, device="cuda"))


def test_flip_test_merge_with_center_scale_equals_get_final_preds():
    hm = torch.from_numpy(_maps(4, 17, 96, 72, 11)).cuda()
    c = torch.tensor([[100.0, 200.0], [640.5, 360.25], [10.0, 700.0], [1000.0, 20.0]])
    s = torch.tensor([[1.2, 1.6], [0.5, 0.67], [2.0, 2.6], [0.9, 1.2]])
    for shift in (False, True):
        merged, preds, maxvals = ops.flip_test_merge(hm, shift_heatmap=shift, center=c, scale=s)
        p2, m2 = ops.get_final_preds(merged, c, s)
        assert torch.equal(preds, p2) and torch.equal(maxvals, m2)


def test_flip_test_merge_other_pairs_and_checks():
    hm = _maps(2, 6, 7, 9, 3)
    _merge_and_compare(hm, True, pairs=[[0, 5], [2, 3]])
    with pytest.raises(ValueError):
        ops.flip_test_merge(torch.from_numpy(hm).cuda(), [[0, 6]])
    with pytest.raises(ValueError):
        ops.flip_test_merge(torch.from_numpy(hm[:3]).cuda(), [])        # odd batch
    with pytest.raises(ValueError):
        ops.flip_test_merge(torch.from_numpy(hm).cuda(), [], center=torch.zeros(2, 2))


# ---- the model ----------------------------------------------------------------------------------------------------------
def _model(cfg):
    m = OTPose(cfg)
    S.fill_synthetic_(m)
    return m.cuda().eval()


def _video_inputs(cfg, B=2, seed=8):
    w_img, h_img = cfg.MODEL.IMAGE_SIZE
    f = cfg.MODEL.get("WINDOW_FRAMES", 5)
    pool = _pool(9, 90, 130, seed)
    c, s = C.box_to_center_scale([[30.0, 10.0, 40.0, 60.0], [70.5, 40.2, 50.0, 45.0]][:B], w_img / h_img, 1.25)
    fi = np.random.RandomState(seed).randint(0, 9, (B, f))
    _, margin = S.synthetic_clip(B, (w_img, h_img), frames=f)
    return torch.from_numpy(pool).cuda(), fi, c, s, margin


# fp16: test_gpu_h16_engine.py's bound (8e-3 of max(1, max |reference|)); fp32: smoke()'s 1e-3
CASES = {"fp32": ((8, (64, 96), 5, "fp32"), 1e-3), "fp16": ((16, (128, 192), 5, "fp16"), 8e-3),
         "fp32_w7": ((8, (64, 96), 7, "fp32"), 1e-3)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_predict_flip_test_equals_restatement_of_the_same_engine(case):
    (width, size, frames, dtype), tol = CASES[case]
    cfg = tiny_cfg(width, size, frames=frames, dtype=dtype)
    model = _model(cfg)
    pool, fi, c, s, margin = _video_inputs(cfg)
    M = C.crop_matrix(c, s, 0.0, size)
    with torch.no_grad():
        plain_before = model.predict(pool, fi, c, s, margin)
        pair = ops.crop_clips(pool, fi, M, size=size, mirror_pair=True)
        plain = ops.crop_clips(pool, fi, M, size=size)
        out = model(pair, margin=torch.cat([margin, margin]).cuda())[0]
        for shift in (False, True):
            preds, maxvals = model.predict(pool, fi, c, s, margin, flip_test=True, shift_heatmap=shift)
            want = R.flip_merge(out.cpu().numpy(), PERM, shift)
            p2, m2 = ops.get_final_preds(torch.from_numpy(want).cuda(), torch.from_numpy(c), torch.from_numpy(s))
            assert torch.equal(preds, p2) and torch.equal(maxvals, m2), shift
            merged = model.flip_test_heatmaps(plain, margin, shift_heatmap=shift)
            assert torch.equal(merged.cpu(), torch.from_numpy(want)), shift
        plain_after = model.predict(pool, fi, c, s, margin)
        # flip_test=False is today's predict: the forward of the plain crops, get_final_preds of its output
        ref_plain = ops.get_final_preds(model(plain, margin=margin.cuda())[0], torch.from_numpy(c), torch.from_numpy(s))
    for a, b in zip(plain_before, plain_after):
        assert torch.equal(a, b)
    for a, b in zip(plain_before, ref_plain):
        assert torch.equal(a, b)
    # the merged maps against the oracle's forwards of x and x.flip(3), merged in numpy
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    x, cfg32 = plain.cpu(), tiny_cfg(width, size, frames=frames)
    ref = R.flip_merge(torch.cat([O.otpose_forward(sd, cfg32, x, margin)[0],
                                  O.otpose_forward(sd, cfg32, x.flip(3), margin)[0]]).numpy(), PERM, True)
    got = model.flip_test_heatmaps(plain, margin.cuda(), shift_heatmap=True).cpu().numpy()
    err = float(np.abs(got - ref).max())
    print(f"{case}: flip-test heat-maps vs oracle max abs err {err:.2e} (range {float(np.abs(ref).max()):.3f})")
    assert err <= tol * max(1.0, float(np.abs(ref).max()))


def test_flip_test_refuses_train_mode():
    cfg = tiny_cfg(8, (64, 96))
    model = _model(cfg).train()
    pool, fi, c, s, margin = _video_inputs(cfg)
    with pytest.raises(RuntimeError):
        model.predict(pool, fi, c, s, margin, flip_test=True)
    with pytest.raises(RuntimeError):
        model.flip_test_heatmaps(torch.zeros((2, 15, 96, 64), device="cuda"), margin)
