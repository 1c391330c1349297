"""Person detector on the GPU (csrc/detect.hip, otpose_amd/detector.py) against the restatement tests/detector_ref.py and
the vectors the reference produced (tests/golden/detector.npz).

Bounds.  Forward and decode: ``E`` is the float32 restatement's largest error against the float64 restatement on the same
weights, relative to the range of the compared tensor (a head map, or the xy / wh / conf-and-class columns of the
prediction); the GPU result must lie within ``4 E`` of the float64 one - the factor allows another summation order and the
folded BatchNorm.  Against the stored float32 reference output the bound is ``5 E``: that output is itself within ``E`` of
the float64 one.  NMS: count, keep order, class and conf equal; merged boxes within 1e-3 px (float32 weighted sums of at
most 32 terms at coordinates up to 416, in another order); frame-pixel boxes within 1e-9 relative of the float64 formulas
over the kernel's own float32 rows.  Letterbox: a correctly rounded level of the exact float64 area mean, up to the
direction of a tie.

Measured on the MI355X: see DESIGN.md section 3.12."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from otpose_amd import detector as DET
from otpose_amd import ops
from tests import detector_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL_CFG = os.path.join(GOLDEN, "detector_small.cfg")
SMALL_IMG, SMALL_SEED, SMALL_INPUT_SEED = 64, 20, 21
DEV = "cuda:0"
COLS = (("xy", slice(0, 2)), ("wh", slice(2, 4)), ("conf, cls", slice(4, None)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "detector.npz"))


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (b.max() - b.min()))


def check_4e(name, gpu, f32, f64, factor=4.0, against=None):
    """``gpu`` within ``factor * E`` of ``against`` (default: the float64 result), E = the float32 restatement's error."""
    e = rel_err(f32, f64)
    got = rel_err(gpu, f64 if against is None else against)
    print(f"{name}: E = {e:.3e}, GPU = {got:.3e} ({got / e:.2f} E)")
    assert e > 0 and got <= factor * e, f"{name}: GPU {got:.3e} > {factor} x E = {factor * e:.3e}"


def small_input():
    return torch.from_numpy(np.random.RandomState(SMALL_INPUT_SEED).uniform(0, 1, (2, 3, SMALL_IMG, SMALL_IMG)).astype(np.float32))


@pytest.fixture(scope="module")
def small():
    blocks = DET.parse_darknet_cfg(SMALL_CFG)[1:]
    sd = R.build_weights(blocks, SMALL_SEED)
    model = DET.PersonDetector(SMALL_CFG, img_size=SMALL_IMG)
    model.load_state_dict(sd)
    p32, h32 = R.forward(blocks, sd, small_input(), SMALL_IMG)
    p64, h64 = R.forward(blocks, sd, small_input(), SMALL_IMG, torch.float64)
    return dict(model=model.to(DEV), p32=p32, h32=h32, p64=p64, h64=h64)


def test_small_net_forward(small, golden):
    pred, heads = small["model"](small_input().to(DEV), return_heads=True)
    assert pred.shape == small["p32"].shape and len(heads) == 2
    for i, h in enumerate(heads):
        check_4e(f"head map {i}", h.cpu(), small["h32"][i], small["h64"][i])
    for name, c in COLS:
        check_4e(f"prediction {name}", pred[..., c].cpu(), small["p32"][..., c], small["p64"][..., c])
        check_4e(f"prediction {name} vs the stored reference output", pred[..., c].cpu(), small["p32"][..., c],
                 small["p64"][..., c], factor=5.0, against=golden["small_pred"][..., c])
    # the decode alone, on the GPU's own head maps: the rows of each layer in the order (anchor, gy, gx)
    blocks = [d for d in small["model"].module_defs if d["type"] == "yolo"]
    off = 0
    for h, d in zip(heads, blocks):
        rows = ops.yolo_decode(h, d["_anchors"], d["_classes"], SMALL_IMG)
        assert torch.equal(rows, pred[:, off:off + rows.shape[1]])
        want32 = R.decode(h.cpu(), d["_anchors"], d["_classes"], SMALL_IMG)
        want64 = R.decode(h.cpu().double(), d["_anchors"], d["_classes"], SMALL_IMG)
        for name, c in COLS:
            check_4e(f"decode of grid {h.shape[2]} {name}", rows[..., c].cpu(), want32[..., c], want64[..., c])
        off += rows.shape[1]
    # a second batch size builds a second engine
    one = small["model"](small_input()[:1].to(DEV))
    for name, c in COLS:
        check_4e(f"batch 1 prediction {name}", one[..., c].cpu(), small["p32"][:1, :, c], small["p64"][:1, :, c])


def test_load_state_dict_invalidates_the_packed_weights(small):
    model, x = small["model"], small_input().to(DEV)
    before = model(x)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    changed = dict(sd)
    changed["module_list.0.conv_0.weight"] = sd["module_list.0.conv_0.weight"] * 0.5
    model.load_state_dict(changed)
    assert not torch.equal(model(x), before)
    model.load_state_dict(sd)
    assert torch.equal(model(x), before)


def test_yolov3_416_forward():
    blocks = DET.yolov3_defs()[1:]
    sd = R.build_weights(blocks, 7)
    x = torch.from_numpy(np.random.RandomState(8).uniform(0, 1, (1, 3, 416, 416)).astype(np.float32))
    p32, _ = R.forward(blocks, sd, x, 416)
    p64, _ = R.forward(blocks, sd, x, 416, torch.float64)
    model = DET.PersonDetector()
    model.load_state_dict(sd)
    pred = model.to(DEV)(x.to(DEV)).cpu()
    assert pred.shape == (1, 10647, 85) and bool(torch.isfinite(pred).all())
    for name, c in COLS:
        check_4e(f"yolov3 416 {name}", pred[..., c], p32[..., c], p64[..., c])


@pytest.mark.parametrize("shape", [(2, 5, 7, 13), (1, 3, 13, 13), (2, 4, 6, 8), (1, 70, 26, 26)])
@pytest.mark.parametrize("up", [1, 2])
def test_leaky_pass(shape, up):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(n * 1000 + c * 100 + h * 10 + w)
    src = torch.randn((n, c + 3, h, w), generator=g).to(DEV)              # the input is channels [2, 2 + c) of src
    sc = torch.randn((n, c + 1, h, w), generator=g).to(DEV)
    for leaky, short in ((True, True), (True, False), (False, True), (False, False)):
        out = torch.full((n, c + 2, h * up, w * up), 7.0, device=DEV)
        ops.leaky_pass(ops.View(src, 2, c), ops.View(out, 1, c), ops.View(sc, 1, c) if short else None, leaky, up)
        want = src[:, 2:2 + c]
        want = torch.nn.functional.leaky_relu(want, 0.1) if leaky else want
        want = want + sc[:, 1:1 + c] if short else want
        want = torch.nn.functional.interpolate(want, scale_factor=up, mode="nearest") if up > 1 else want
        assert torch.equal(out[:, 1:1 + c], want)
        assert bool((out[:, 0] == 7.0).all()) and bool((out[:, -1] == 7.0).all())   # the neighbouring channels are untouched


@pytest.mark.parametrize("case", ["pair", "edge", "single", "large"])
def test_box_nms_merge(golden, case):
    pred = torch.from_numpy(golden[f"nms_{case}_pred"])
    conf_thres, nms_thres = (float(v) for v in golden["nms_thresholds"])
    want = R.nms(pred, conf_thres, nms_thres)
    stored, stored_n = golden[f"nms_{case}_dets"], golden[f"nms_{case}_counts"]
    for frame in (None, (100, 180), (181, 96), (256, 256)):
        counts, dets, pcounts, pboxes, pscores = ops.box_nms_merge(pred.to(DEV), conf_thres, nms_thres, frame, 416, 0)
        counts, dets, pcounts, pboxes, pscores = (t.cpu() for t in (counts, dets, pcounts, pboxes, pscores))
        assert dets.shape == (pred.shape[0], pred.shape[1], 6) and pboxes.dtype == torch.float64
        for i, w in enumerate(want):
            k = 0 if w is None else len(w)
            assert int(counts[i]) == k == stored_n[i]
            assert bool((dets[i, k:] == 0).all())                                   # no stale rows
            if k:
                got = dets[i, :k]
                assert torch.equal(got[:, 4:], w[:, 4:])                            # keep order (conf) and class
                assert np.array_equal(got[:, 4:].numpy(), stored[i, :k, 4:])
                assert float((got[:, :4] - w[:, :4]).abs().max()) <= 1e-3
                assert float(np.abs(got[:, :4].numpy() - stored[i, :k, :4]).max()) <= 1e-3
            # persons: the float64 formulas over the kernel's own rows
            person = dets[i, :k][dets[i, :k, 5] == 0] if k else dets[i, :0]
            assert int(pcounts[i]) == len(person)
            kp = len(person)
            assert bool((pboxes[i, kp:] == 0).all()) and bool((pscores[i, kp:] == 0).all())
            if kp:
                if frame is None:
                    ref = person[:, :4].double().numpy().copy()
                    ref[:, 2:] -= ref[:, :2]
                else:
                    ref = R.rescale(person.numpy(), frame, 416)
                assert np.abs(pboxes[i, :kp].numpy() - ref).max() <= 1e-9 * np.abs(ref).max()
                assert torch.equal(pscores[i, :kp], person[:, 4])


@pytest.mark.parametrize("hw", [(100, 180), (181, 96), (256, 256)])
def test_letterbox(hw):
    size = 64
    frames = np.random.RandomState(hw[0]).randint(0, 256, (2,) + hw + (3,)).astype(np.uint8)
    out = ops.letterbox(torch.from_numpy(frames).to(DEV), size).cpu().numpy().astype(np.float64)
    assert out.shape == (2, 3, size, size)
    lv = out * 255.0
    assert np.abs(lv - np.rint(lv)).max() <= 1e-7 * 255.0                            # a multiple of 1 / 255
    mean, pad = R.letterbox64(frames, size)
    assert np.abs(out - mean / 255.0).max() <= (0.5 + 1e-3) / 255.0                  # a correctly rounded level
    assert pad.any() == (hw[0] != hw[1])
    assert np.all(out[:, :, pad].astype(np.float32) == np.float32(127) / np.float32(255))
    rounded = R.levels(mean)
    ties = np.abs(mean - np.floor(mean) - 0.5) < 1e-9
    assert np.array_equal(np.rint(lv)[~ties], rounded[~ties])


def test_letterbox_refuses_to_enlarge():
    with pytest.raises(ValueError):
        ops.letterbox(torch.zeros((2, 40, 50, 3), dtype=torch.uint8, device=DEV), 64)
    with pytest.raises(TypeError):
        ops.letterbox(torch.zeros((2, 100, 180, 3), dtype=torch.float32, device=DEV), 64)


def test_detect_end_to_end(small):
    model = small["model"]
    frames = torch.from_numpy(np.random.RandomState(4).randint(0, 256, (2, 100, 180, 3)).astype(np.uint8)).to(DEV)
    boxes, scores, counts = model.detect(frames)
    x = ops.letterbox(frames, SMALL_IMG)
    pred = model(x)
    _, _, pcounts, pboxes, pscores = ops.box_nms_merge(pred, model.conf_thres, model.nms_thres, (100, 180), SMALL_IMG, 0)
    k = int(pcounts.max())
    assert k > 0 and boxes.shape == (2, k, 4) and boxes.dtype == torch.float64 and boxes.is_cuda
    assert torch.equal(counts, pcounts) and torch.equal(boxes, pboxes[:, :k]) and torch.equal(scores, pscores[:, :k])
    lists = model.detect_list(frames)
    assert isinstance(lists, list) and len(lists) == 2
    for i, cands in enumerate(lists):
        assert isinstance(cands, list) and len(cands) == int(counts[i])
        for j, c in enumerate(cands):
            assert isinstance(c, list) and len(c) == 4 and all(isinstance(v, float) for v in c)
            assert c == boxes[i, j].tolist()
