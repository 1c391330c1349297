"""Weight EMA without a GPU: the arithmetic the kernels are held to (tests/ema_ref.py against the reference class's recorded
states, tests/golden/ema.npz), what ``ModelEma`` refuses, the argument checks of the C entry points, and the checkpoint entry."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import ema_ref as R
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def fixture():
    return R.load(np.load(os.path.join(GOLDEN, "ema.npz")))


def test_fixture_holds_what_the_kernels_must_survive(fixture):
    keys, start, srcs, emas = fixture
    sizes = sorted(start[k].size for k in keys if k.startswith("p"))
    assert sizes == [1, 3, 63, 64, 65, 1025, 4099]
    counters = [k for k in keys if start[k].dtype == np.int64]
    assert len(counters) == 2 and len([k for k in keys if "running_" in k]) == 4
    allv = np.concatenate([s[k].reshape(-1) for s in [start] + srcs for k in keys if s[k].dtype == np.float32])
    mag = np.abs(allv[allv != 0])
    assert mag.min() < 1.2e-38 and mag.max() >= 1e30                       # subnormals up to 1e30
    assert np.any((allv == 0) & np.signbit(allv)) and np.any((allv == 0) & ~np.signbit(allv))
    assert all(0 <= int(s[k]) < 2 ** 24 for s in [start] + srcs for k in counters)
    assert int(start["bn1.num_batches_tracked"]) == 1000 and int(srcs[0]["bn1.num_batches_tracked"]) == 1001


@pytest.mark.parametrize("decay", R.DECAYS)
def test_restatement_reproduces_the_reference_bit_for_bit(fixture, decay):
    keys, start, srcs, emas = fixture
    cur = {k: v.copy() for k, v in start.items()}
    for i, src in enumerate(srcs):
        for k in keys:
            cur[k] = R.ema_update(cur[k], src[k], decay)
            assert R.same_bits(cur[k], emas[decay][i][k]), (decay, i + 1, k)


def test_truncation_and_the_unfused_sum_show_in_the_fixture(fixture):
    """The cases that tell the specified arithmetic from its neighbours are really in the file."""
    keys, start, srcs, emas = fixture
    # 0.999 * 1000 + 0.001 * 1001 = 1000.001 -> 1000 either way; 0.999 * 1000 + 0.001 * 999 = 999.999 -> 999 only by truncation
    assert int(emas[0.999][0]["bn1.num_batches_tracked"]) == 1000 and int(emas[0.999][3]["bn1.num_batches_tracked"]) == 999
    rounded_differs = 0
    for decay in R.DECAYS:
        d, omd = R.scalars(decay)
        for k in ("bn1.num_batches_tracked", "bn2.num_batches_tracked"):
            prev = start[k]
            for i, src in enumerate(srcs):
                r = np.float32(np.float32(d * np.float32(prev)) + np.float32(omd * np.float32(src[k])))
                rounded_differs += int(np.rint(r)) != int(emas[decay][i][k])
                prev = emas[decay][i][k]
    assert rounded_differs >= 3
    # a fused multiply-add (either product kept exact) changes bits somewhere in the large tensors
    d, omd = R.scalars(0.999)
    e, m = start["p4099"].astype(np.float64), srcs[0]["p4099"].astype(np.float64)
    with np.errstate(all="ignore"):
        fused = (np.float64(d) * e + (np.float64(omd) * m).astype(np.float32).astype(np.float64)).astype(np.float32)
    assert not R.same_bits(fused, emas[0.999][0]["p4099"])
    # decay 0 is not a plain copy: +0 * ema + 1 * (-0) is +0
    src, out = srcs[1]["p4099"], emas[0.0][1]["p4099"]
    turned = (src == 0) & np.signbit(src) & ~np.signbit(out)
    assert turned.any() and not R.same_bits(src, out)


class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(3, 2)
        self.bn = torch.nn.BatchNorm1d(2)


def test_model_ema_rejects_another_device_and_half_precision():
    from otpose_amd import ModelEma
    net = _Small()
    with pytest.raises(NotImplementedError):
        ModelEma(net, device="cpu")
    with pytest.raises(NotImplementedError):
        ModelEma(net, decay=0.9, device=torch.device("cpu"))
    for dt in (torch.float16, torch.bfloat16):
        half = _Small()
        half.fc.to(dt)
        with pytest.raises(TypeError, match="fc.weight"):
            ModelEma(half)
    ema = ModelEma(net, decay=0.5)                                           # the reference's attributes
    assert ema.decay == 0.5 and ema.device is None and not ema.module.training and ema.module is not net
    assert list(ema.module.state_dict()) == list(net.state_dict())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ema.update(net)


def test_entry_points_check_their_arguments():
    from otpose_amd import hip
    L = hip.lib()
    F32, I64 = hip.CONSTANTS["OTP_DTYPE_F32"], hip.CONSTANTS["OTP_DTYPE_I64"]
    BAD, UNS = hip.CONSTANTS["OTP_ERR_BAD_ARG"], hip.CONSTANTS["OTP_ERR_UNSUPPORTED"]
    assert I64 not in (F32, hip.CONSTANTS["OTP_DTYPE_F16"], hip.CONSTANTS["OTP_DTYPE_BF16"], hip.CONSTANTS["OTP_DTYPE_F64"])
    p = ctypes.c_void_p
    assert L.otp_ema_update(None, p(64), 4, 0.5, 0.5, None) == BAD
    assert L.otp_ema_update(p(64), None, 4, 0.5, 0.5, None) == BAD
    assert L.otp_ema_update(p(66), p(64), 4, 0.5, 0.5, None) == UNS           # not 4-byte aligned
    assert L.otp_ema_update(p(64), p(64), 0, 0.5, 0.5, None) == 0             # nothing to do: no launch
    assert L.otp_ema_update_table(None, 3, 0.5, 0.5, None) == BAD
    assert L.otp_ema_update_table(p(64), -1, 0.5, 0.5, None) == BAD
    assert L.otp_ema_update_table(None, 0, 0.5, 0.5, None) == 0
    nb = L.otp_ema_job_bytes()
    assert 0 < nb <= 64 and nb % 8 == 0
    a, b = ctypes.create_string_buffer(nb), ctypes.create_string_buffer(nb)
    assert L.otp_ema_job(None, p(64), 4, F32, None, a) == BAD
    assert L.otp_ema_job(p(64), None, 4, F32, None, a) == BAD
    assert L.otp_ema_job(p(64), p(128), 4, F32, None, None) == BAD
    for code in (hip.CONSTANTS["OTP_DTYPE_F16"], hip.CONSTANTS["OTP_DTYPE_F64"], 17, -1):
        assert L.otp_ema_job(p(64), p(128), 4, code, None, a) == UNS
    assert L.otp_ema_job(p(68), p(128), 1, I64, None, a) == UNS               # int64 needs 8-byte alignment
    assert L.otp_ema_job(p(68), p(132), 5000, F32, None, a) == 0
    assert L.otp_ema_job(p(64), p(128), 1, I64, a, b) == 0
    assert a.raw != b.raw


def test_checkpoint_round_trip_with_and_without_the_average(tmp_path):
    from otpose_amd import ModelEma, checkpoints as C
    torch.manual_seed(3)
    net = _Small()
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    ema = ModelEma(net)
    with torch.no_grad():
        for v in ema.module.state_dict().values():
            v.copy_(torch.full_like(v, 7))
    plain = torch.load(C.save_checkpoint(3, str(tmp_path / "plain"), net, opt, global_steps=11), weights_only=False)
    assert sorted(plain) == ["begin_epoch", "optimizer", "state_dict", "tensorboard_global_steps"]      # the key set of always
    path = C.save_checkpoint(3, str(tmp_path / "ema"), net, opt, global_steps=11, model_ema=ema)
    with_ema = torch.load(path, weights_only=False)
    assert sorted(with_ema) == sorted(list(plain) + ["state_dict_ema"])
    assert list(with_ema["state_dict_ema"]) == list(net.state_dict())
    best = torch.load(C.save_best_checkpoint(3, str(tmp_path / "ema"), net, opt, 81.5, model_ema=ema), weights_only=False)
    assert "state_dict_ema" in best
    # nn.DataParallel's prefix is stripped from the average's keys as from the model's
    dp = ModelEma(torch.nn.DataParallel(_Small()))
    assert all(k.startswith("module.") for k in dp.module.state_dict())
    assert list(C._checkpoint_dict(1, net, opt, 0, dp)["state_dict_ema"]) == list(net.state_dict())
    # resume: the model, and the copy from its own entry
    net2 = _Small()
    ema2 = ModelEma(net2)
    _, _, epoch, extra = C.resume(net2, torch.optim.SGD(net2.parameters(), lr=0.1), path, model_ema=ema2)
    assert epoch == 4 and extra == {"tensorboard_global_steps": 11}
    for (k, a), b in zip(net.state_dict().items(), net2.state_dict().values()):
        assert torch.equal(a, b), k
    for k, v in ema2.module.state_dict().items():
        assert torch.equal(v, torch.full_like(v, 7)), k
    # a file without the entry loads as before and leaves the copy alone; a file with it loads without a ModelEma
    ema3 = ModelEma(_Small())
    before = {k: v.clone() for k, v in ema3.module.state_dict().items()}
    C.resume(_Small(), None, str(tmp_path / "plain" / "epoch_3_state.pth"), model_ema=ema3)
    assert all(torch.equal(v, before[k]) for k, v in ema3.module.state_dict().items())
    C.resume(_Small(), None, path)
