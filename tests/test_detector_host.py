"""Person detector, host side: the cfg parser, the built-in YOLOv3 layer list, the ``state_dict`` layout and the Darknet
weights format of ``otpose_amd.detector`` against what the reference produced (tests/golden/detector.npz, written by
tests/golden/make_golden_detector.py), and the restatement tests/detector_ref.py against the same vectors - the GPU tests
measure the kernels against that restatement.

Bounds.  ``E`` is the float32 restatement's largest error against the same restatement in float64, relative to the range
of the compared tensor; a float32 result must lie within ``4 E`` of the float64 one (the factor allows another summation
order).  The recorded frame-pixel boxes were evaluated by numpy scalars, which stay float32 under numpy >= 2: they get
``8 * 2^-24`` of the frame size on top (eight float32 roundings between the corners and the box)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

from otpose_amd import detector as DET
from tests import detector_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL_CFG = os.path.join(GOLDEN, "detector_small.cfg")
SMALL_IMG, SMALL_SEED, SMALL_INPUT_SEED = 64, 20, 21
NMS_CASES = ("pair", "edge", "single", "large")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "detector.npz"))


def small_input():
    return torch.from_numpy(np.random.RandomState(SMALL_INPUT_SEED).uniform(0, 1, (2, 3, SMALL_IMG, SMALL_IMG)).astype(np.float32))


def rel_err(a, b):
    """max |a - b| over the range of b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (b.max() - b.min()))


def test_parse_small_cfg(golden):
    assert DET.parse_darknet_cfg(SMALL_CFG) == json.loads(str(golden["small_parse"]))


def test_yolov3_defs_equal_reference_cfg(golden):
    want = json.loads(str(golden["yolov3_parse"]))
    got = DET.yolov3_defs()
    assert len(got) == len(want) == 108
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"block {i}"
    other = DET.yolov3_defs(num_classes=3, img_size=320)
    assert other[0]["width"] == other[0]["height"] == "320"
    assert [d["filters"] for d in other if d.get("activation") == "linear" and d["type"] == "convolutional"] == ["24"] * 3
    assert all(d["classes"] == "3" for d in other if d["type"] == "yolo")


@pytest.mark.parametrize("which", ["small", "yolov3"])
def test_state_dict_manifest(golden, which):
    m = DET.PersonDetector(SMALL_CFG, img_size=SMALL_IMG) if which == "small" else DET.PersonDetector()
    want = json.loads(str(golden[which + "_manifest"]))
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert sorted(got) == sorted(want)
    assert got == want


def test_maxpool_is_refused(tmp_path):
    cfg = tmp_path / "tiny.cfg"
    cfg.write_text("[net]\nwidth=64\nheight=64\nchannels=3\n\n[convolutional]\nbatch_normalize=1\nfilters=8\nsize=3\nstride=1\n"
                   "pad=1\nactivation=leaky\n\n[maxpool]\nsize=2\nstride=2\n")
    with pytest.raises(NotImplementedError, match=r"block 1 \[maxpool\]"):
        DET.PersonDetector(str(cfg), img_size=64)


def test_darknet_weights_round_trip(tmp_path):
    m = DET.PersonDetector(SMALL_CFG, img_size=SMALL_IMG)
    blocks = DET.parse_darknet_cfg(SMALL_CFG)[1:]
    sd = R.build_weights(blocks, 3)
    # the file, written here in the format: 5 int32, then per conv BN bias, weight, mean, var (or the conv bias), conv weights
    path = tmp_path / "small.weights"
    with open(path, "wb") as f:
        np.array([0, 2, 0, 1234, 0], np.int32).tofile(f)
        for i, _, d in R.conv_blocks(blocks):
            if int(d["batch_normalize"]):
                for k in ("bias", "weight", "running_mean", "running_var"):
                    sd[f"module_list.{i}.batch_norm_{i}.{k}"].numpy().tofile(f)
            else:
                sd[f"module_list.{i}.conv_{i}.bias"].numpy().tofile(f)
            sd[f"module_list.{i}.conv_{i}.weight"].numpy().tofile(f)
    m.load_darknet_weights(str(path))
    got = m.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    assert m.header_info[3] == 1234
    again = tmp_path / "again.weights"
    m.save_darknet_weights(str(again))
    assert again.read_bytes() == path.read_bytes()
    with open(path, "ab") as f:
        np.zeros(1, np.float32).tofile(f)
    with pytest.raises(ValueError):
        m.load_darknet_weights(str(path))


def test_cpu_tensors_raise():
    m = DET.PersonDetector(SMALL_CFG, img_size=SMALL_IMG)
    with pytest.raises(NotImplementedError):
        m(small_input())
    with pytest.raises(NotImplementedError):
        m.detect(torch.zeros((1, 100, 180, 3), dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        m.train()


def test_ref_forward_reproduces_golden(golden):
    blocks = DET.parse_darknet_cfg(SMALL_CFG)[1:]
    sd = R.build_weights(blocks, SMALL_SEED)
    p32, _ = R.forward(blocks, sd, small_input(), SMALL_IMG)
    p64, _ = R.forward(blocks, sd, small_input(), SMALL_IMG, torch.float64)
    want = golden["small_pred"]
    assert p32.shape == want.shape == (2, 3 * 16 * 16 + 3 * 32 * 32, 8)
    for name, cols in (("box", slice(0, 4)), ("conf, cls", slice(4, 8))):
        e = rel_err(p32[..., cols], p64[..., cols])
        got = rel_err(want[..., cols], p64[..., cols])
        print(f"{name}: E = {e:.3e}, reference vs float64 = {got:.3e}")
        assert 0 < e < 1e-5 and got <= 4 * e


@pytest.mark.parametrize("case", NMS_CASES)
def test_ref_nms_reproduces_golden(golden, case):
    pred = torch.from_numpy(golden[f"nms_{case}_pred"])
    conf_thres, nms_thres = golden["nms_thresholds"]
    d32 = R.nms(pred, conf_thres, nms_thres)
    d64 = R.nms(pred.double(), conf_thres, nms_thres)
    want, counts = golden[f"nms_{case}_dets"], golden[f"nms_{case}_counts"]
    for i, (a, b) in enumerate(zip(d32, d64)):
        assert (0 if a is None else len(a)) == counts[i]
        if a is None:
            continue
        w = want[i, :counts[i]]
        assert np.array_equal(a[:, 4:].numpy(), w[:, 4:])                   # keep order (conf), class
        assert np.array_equal(b[:, 5].numpy(), w[:, 5])
        e = float((a[:, :4].double() - b[:, :4]).abs().max()) / 416.0
        got = float(np.abs(w[:, :4] - b[:, :4].numpy()).max()) / 416.0
        print(f"{case}[{i}]: E = {e:.3e}, reference vs float64 = {got:.3e}")
        assert got <= 4 * e + 1e-12


def test_ref_rescale_reproduces_golden(golden):
    pred = torch.from_numpy(golden["nms_pair_pred"][:1])
    conf_thres, nms_thres = golden["nms_thresholds"]
    d32 = R.nms(pred, conf_thres, nms_thres)[0]
    d64 = R.nms(pred.double(), conf_thres, nms_thres)[0]
    e = float((d32[:, :4].double() - d64[:, :4]).abs().max()) / 416.0
    for i, (h, w) in enumerate(golden["rescale_frames"]):
        want = golden[f"rescale_{i}"]
        got = R.rescale(d32.numpy(), (h, w), 416)
        assert got.shape == want.shape and got.dtype == np.float64
        bound = (4 * e + 8 * 2.0 ** -24) * max(h, w)
        assert np.abs(got - want).max() <= bound, (h, w, np.abs(got - want).max(), bound)


def test_letterbox64_is_an_area_mean(golden):
    assert golden["pad_level"][0] == 127
    rs = np.random.RandomState(2)
    f = rs.randint(0, 256, (1, 256, 256, 3)).astype(np.uint8)
    mean, pad = R.letterbox64(f, 64)                                   # integer scale 4: the plain 4 x 4 block mean
    want = f[0].reshape(64, 4, 64, 4, 3).astype(np.float64).mean(axis=(1, 3)).transpose(2, 0, 1)
    assert np.abs(mean[0] - want).max() < 1e-9 and not pad.any()
    f = rs.randint(0, 256, (1, 100, 180, 3)).astype(np.uint8)
    mean, pad = R.letterbox64(f, 64)
    assert pad[:14].all() and pad[-14:].all() and not pad[15:49].any()  # 40 pad rows of 180 each side = 14.2 output rows
    assert np.all(mean[0][:, pad] == 127.0)
    assert abs(mean[0].sum() * (180 / 64) ** 2 - (f[0].astype(np.float64).sum() + 127.0 * 80 * 180 * 3)) < 1e-3
