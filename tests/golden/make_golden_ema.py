#!/usr/bin/env python
"""Generate tests/golden/ema.npz by running the reference's ``ModelEma`` on the CPU (build container only).

Run from the repo root:  ``python tests/golden/make_golden_ema.py``

thirdparty/utils/train_utils.py:240-262 over a small module: float32 parameters of 1, 3, 63, 64, 65, 1025 and 4099 elements
(the scalar head and tail and the 16-byte body of the kernels) and two BatchNorm layers (running statistics and the int64
``num_batches_tracked``).  Values: signs and magnitudes from 1e-30 to 1e30, with +-0, subnormals and values whose products
become subnormal planted at the front of every float tensor; the counters stay below 2^24 and step through pairs where the
truncation of the float result matters (1000 against 1001).  Stored, as ``<state>/<state_dict key>``:

    start                                the copy's state before the first update (the same for every decay)
    src1 .. src5                         the model's state at the five consecutive ``update()`` calls
    ema_<decay>_1 .. ema_<decay>_5       the copy's state after each call, decay in 0.999, 0.9, 0.0
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import import_reference          # noqa: E402

SIZES = (1, 3, 63, 64, 65, 1025, 4099)
DECAYS = (0.999, 0.9, 0.0)
SPECIAL = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -3e-39, 1.2e-38, -1.3e-38, 1e-30, -1e30, 1e30, 1.0]
COUNTERS = {"bn1.num_batches_tracked": (1000, [1001, 1001, 1003, 999, 0]),
            "bn2.num_batches_tracked": (0, [1, 2, 16777215, 5, 123457])}


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        for n in SIZES:
            setattr(self, f"p{n}", torch.nn.Parameter(torch.zeros(n)))
        self.bn1 = torch.nn.BatchNorm1d(17)
        self.bn2 = torch.nn.BatchNorm2d(40)


def values(n, gen):
    """n float32 values: random sign times 10^U(-30, 30), the special values planted at the front (rotated per draw)."""
    mag = torch.rand(n, generator=gen, dtype=torch.float64) * 60 - 30
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    v = (sign * 10.0 ** mag).float()
    rot = int(torch.randint(len(SPECIAL), (1,), generator=gen))
    sp = torch.tensor(SPECIAL[rot:] + SPECIAL[:rot], dtype=torch.float32)
    k = min(n, len(sp))
    if n >= 3:
        v[:k] = sp[:k]
    return v


def state(net, gen, counters):
    sd = {}
    for k, t in net.state_dict().items():
        if t.dtype == torch.int64:
            sd[k] = torch.tensor(counters[k], dtype=torch.int64)
        else:
            sd[k] = values(t.numel(), gen).reshape(t.shape)
    return sd


def main():
    import_reference()
    from thirdparty.utils.train_utils import ModelEma
    gen = torch.Generator().manual_seed(20240607)
    net = Net()
    start = state(net, gen, {k: v[0] for k, v in COUNTERS.items()})
    srcs = [state(net, gen, {k: v[1][i] for k, v in COUNTERS.items()}) for i in range(5)]
    out = {}
    for k, v in start.items():
        out["start/" + k] = v.numpy().copy()
    for i, s in enumerate(srcs):
        for k, v in s.items():
            out[f"src{i + 1}/{k}"] = v.numpy().copy()
    for decay in DECAYS:
        net.load_state_dict(start)
        ema = ModelEma(net, decay=decay)
        for i, s in enumerate(srcs):
            net.load_state_dict(s)
            ema.update(net)
            for k, v in ema.module.state_dict().items():
                out[f"ema_{decay}_{i + 1}/{k}"] = v.detach().numpy().copy()
    path = os.path.join(HERE, "ema.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} kB, {len(out)} arrays)")
    for k in COUNTERS:
        print(" ", k, [int(out[f"ema_{d}_{i}/{k}"]) for d in DECAYS for i in range(1, 6)])


if __name__ == "__main__":
    main()
