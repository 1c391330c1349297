"""``VideoPose`` (otpose_amd/video.py): the device crop plan + the pose network at one fixed batch size, against
``OTPose.predict`` fed the host-built plan (tests/pose_plan_ref.py) - equal bit for bit through the same engine, within the
end-to-end heat-map tolerance through an engine of another batch size - and the engine that is never rebuilt."""
import numpy as np
import pytest
import torch

from otpose_amd import OTPose, VideoPose, ops, tiny_cfg
from otpose_amd import posetrack_eval as PE
from otpose_amd import synthetic as S
from tests import pose_plan_ref as R
from tests.test_gpu_e2e import TOL                       # 1e-3 max-abs on the output heat-maps

pytestmark = pytest.mark.gpu
SIZE = (64, 96)
NF = 7


@pytest.fixture(scope="module")
def model():
    m = OTPose(tiny_cfg(8, SIZE))
    S.fill_synthetic_(m)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def pool():
    return torch.from_numpy(np.random.RandomState(8).randint(0, 256, (NF, 90, 130, 3)).astype(np.uint8)).cuda()


def _detections(counts, seed=2):
    """What a detector would return over the 7-frame pool (one video, frames 0..6): counts[s] boxes in frame s."""
    rng = np.random.RandomState(seed)
    k = max(counts)
    boxes = np.stack([rng.uniform(0, 70, (NF, k)), rng.uniform(0, 30, (NF, k)), rng.uniform(25, 60, (NF, k)),
                      rng.uniform(30, 60, (NF, k))], axis=2)
    scores = rng.uniform(0.5, 1.0, (NF, k)).astype(np.float32)
    counts = np.array(counts, np.int32)
    for s in range(NF):
        boxes[s, counts[s]:], scores[s, counts[s]:] = 0, 0
    return boxes, scores, counts, np.arange(NF, dtype=np.int32), np.full(NF, NF, np.int32)


def _cuda(det):
    return [torch.from_numpy(a).cuda() for a in det]


def _host_plan(det, rows):
    """The host recipe's arguments of ``predict`` for the persons of ``det``, padded to ``rows`` persons with empty crops
    (frame -1; a unit scale, because the host's crop matrix of a zero scale is singular)."""
    total = int(det[2].sum())
    p = R.pose_plan_ref(*det, (0, NF), 0.0, SIZE[0] / SIZE[1], 1.25, SIZE, True, total)
    pad = rows - total
    c = np.concatenate([p["center"], np.zeros((pad, 2), np.float32)])
    s = np.concatenate([p["scale"], np.ones((pad, 2), np.float32)])
    fi = np.concatenate([p["frame_idx"], np.full((pad, 5), -1, np.int32)])
    mg = np.concatenate([p["margin"], np.zeros((pad, 4), np.float32)])
    return p, fi, c, s, torch.from_numpy(mg)


@pytest.mark.parametrize("flip", [False, True])
def test_run_equals_predict_on_the_host_plan_through_the_same_engine(model, pool, flip):
    det = _detections([0, 2, 1, 0, 2, 0, 0])
    vp = VideoPose(model, 8, flip_test=flip, shift_heatmap=flip)
    with torch.no_grad():
        res = vp.run(pool, *_cuda(det))
        engine = model._engine
        p, fi, c, s, mg = _host_plan(det, 8)
        preds, maxvals = model.predict(pool, fi, c, s, mg, flip_test=flip, shift_heatmap=flip)
    assert model._engine is engine and engine.B == (16 if flip else 8)
    assert res.preds.shape == (5, 17, 2) and res.maxvals.shape == (5, 17, 1)
    assert torch.equal(res.preds, preds[:5]) and torch.equal(res.maxvals, maxvals[:5])
    assert np.array_equal(res.center.cpu().numpy(), p["center"]) and np.array_equal(res.scale.cpu().numpy(), p["scale"])
    assert np.array_equal(res.box_score.cpu().numpy(), p["box_score"]) and res.box_score.dtype == torch.float64
    assert res.person_slot.cpu().tolist() == [1, 1, 2, 4, 4] and res.pr_off.cpu().tolist() == [0, 0, 2, 3, 3, 5, 5, 5]


def test_run_against_predict_at_the_exact_person_count(model, pool):
    """Another engine batch (5 instead of 8): the heat-maps agree within the end-to-end tolerance, and VideoPose's keypoints
    are the decode of ITS heat-maps - on the device bit for bit, against the oracle's decode as tests/test_decode.py does."""
    from oracle import otpose_oracle as O
    det = _detections([0, 2, 1, 0, 2, 0, 0])
    with torch.no_grad():
        res = VideoPose(model, 8).run(pool, *_cuda(det))
        p, fi, c, s, mg = _host_plan(det, 8)
        hm8 = model.forward_video(pool, fi, c, s, mg)[0][:5].clone()
        assert model._engine.B == 8
        p5, fi5, c5, s5, mg5 = _host_plan(det, 5)
        hm5 = model.forward_video(pool, fi5, c5, s5, mg5)[0].clone()
        assert model._engine.B == 5
        again, again_v = ops.get_final_preds(hm8, torch.from_numpy(c5), torch.from_numpy(s5))
    err = float((hm8 - hm5).abs().max())
    print("max |heat-maps at batch 8 - at batch 5| = %.3e" % err)
    assert err <= TOL
    assert torch.equal(res.preds, again) and torch.equal(res.maxvals, again_v)
    ref, ref_v = O.get_final_preds(hm8.cpu().numpy(), c5, s5)
    assert np.allclose(res.preds.cpu().numpy(), ref, atol=1e-3) and np.array_equal(res.maxvals.cpu().numpy(), ref_v)


def test_the_engine_is_built_once(model, pool):
    vp = VideoPose(model, 8)
    three, seven = _detections([0, 1, 0, 2, 0, 0, 0], 3), _detections([1, 2, 0, 2, 0, 1, 1], 4)
    with torch.no_grad():
        a = vp.run(pool, *_cuda(three))
        engine = model._engine
        b = vp.run(pool, *_cuda(seven))
        assert model._engine is engine and engine.B == 8
        assert a.preds.shape[0] == 3 and b.preds.shape[0] == 7
        built = []
        for det in (three, seven):                                           # the host recipe: one engine per person count
            _, fi, c, s, mg = _host_plan(det, int(det[2].sum()))
            model.predict(pool, fi, c, s, mg)
            built.append(model._engine)
    assert built[0] is not engine and built[1] is not built[0] and [e.B for e in built] == [3, 7]


def test_eleven_persons_run_as_three_groups_of_four(model, pool):
    det = _detections([2, 3, 0, 1, 2, 0, 3], 5)
    calls = []
    with torch.no_grad():
        vp = VideoPose(model, 4)
        model.input_buffers(4, pool.device)
        engine_run = model._engine.run

        def counted(*a, **k):
            calls.append(1)
            return engine_run(*a, **k)
        model._engine.run = counted
        try:
            res = vp.run(pool, *_cuda(det))
        finally:
            del model._engine.run
        p, fi, c, s, mg = _host_plan(det, 12)
        want = [model.predict(pool, fi[g:g + 4], c[g:g + 4], s[g:g + 4], mg[g:g + 4]) for g in (0, 4, 8)]
    assert len(calls) == 3 and model._engine.B == 4
    assert res.preds.shape == (11, 17, 2) and res.person_slot.cpu().tolist() == [0, 0, 1, 1, 1, 3, 4, 4, 6, 6, 6]
    assert torch.equal(res.preds, torch.cat([w[0] for w in want])[:11])
    assert torch.equal(res.maxvals, torch.cat([w[1] for w in want])[:11])
    assert np.array_equal(res.center.cpu().numpy(), p["center"])
    with pytest.raises(ValueError, match="11.*8"):
        vp.run(pool, *_cuda(det), max_persons=7)                             # rounded up to 8 rows: three persons too few
    empty = vp.run(pool, *_cuda(det), detect=(2, 3))
    assert empty.preds.shape == (0, 17, 2) and empty.pr_off.cpu().tolist() == [0] * 8


def test_outputs_feed_pose_nms_and_the_evaluator_unchanged(model, pool):
    det = _detections([2, 3, 0, 1, 2, 0, 3], 5)
    with torch.no_grad():
        res = VideoPose(model, 4).run(pool, *_cuda(det))
    n = res.preds.shape[0]
    area = (res.scale.double() * 200).prod(1)
    sample = torch.arange(n, dtype=torch.int32, device="cuda")
    keep, score, rank = ops.pose_nms(res.pr_off, sample, res.preds, res.maxvals, res.box_score, area, oks_thresh=0.9)
    assert keep.shape == (n,) and keep.dtype == torch.bool and bool(keep.any()) and bool(torch.isfinite(score).all())
    p = res.preds.cpu().numpy().astype(np.float64)
    slot = res.person_slot.cpu().tolist()

    def person(i):
        q = p[i][list(PE.COCO_OF_OFFICIAL)] + 1.0
        return {"annopoints": [{"point": [{"id": [k], "x": [float(q[k, 0])], "y": [float(q[k, 1])]} for k in range(15)]}],
                "x1": [10.0], "y1": [10.0], "x2": [22.0], "y2": [26.0]}
    frames = [{"annorect": [person(i) for i in range(n) if slot[i] == s]} for s in range(NF)]
    ev = PE.PoseTrackEvaluator(frames, nms=PE.PoseNMS(oks_thresh=0.9))
    ev.add(res.preds, res.maxvals, res.box_score, res.person_slot, scale=res.scale)
    out = ev.summarize()
    assert out["ap"].shape == (16,) and np.isfinite(out["ap"][-1]) and out["ap"][-1] >= 0 and "Mean" in out["table"]
